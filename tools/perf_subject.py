"""Rate of fe_subject_region on a batch of 1024x1024 images, by stage, beside fe_leading_lines at the same shape and a BatchScorer step
with and without subject_region. usage: perf_subject.py [n] [hw] [out]   (default 64 1024 profiles/subject_perf.txt)

Stages are timed through the entry points that run them alone: gray + histogram (fe_image_stats), labelling + external test + border walks
(fe_external_contours on the edge image fe_subject_region returned), the whole call from host memory and from a resident batch. Pure noise
is the stress case: every third pixel is an edge and an image has hundreds of thousands of components; the lane-serial border walk is the
stage to watch there."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from facet_amd import Engine
from facet_amd.batch import BatchScorer
from facet_amd.weights import synthetic_images, synthetic_state_dict
from facet_amd._lib import FE_MODEL_TOPIQ, FE_MODEL_CLIP, FE_MODEL_AESTHETIC, FE_MODEL_U2NETP, FE_MODEL_SAMP

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
hw = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "subject_perf.txt")
lines_out = []


def say(s):
    print(s, flush=True)
    lines_out.append(s)


def timed(f, reps=3):
    f()
    best = 1e30
    for _ in range(reps):
        t0 = time.time(); f(); best = min(best, time.time() - t0)
    return best


e = Engine(0)
rng = np.random.default_rng(0)
yy, xx = np.mgrid[:hw, :hw]
base = (96 + 60 * np.sin(xx / 90.0) + 50 * np.cos(yy / 70.0)).astype(np.int32)
photo = np.empty((n, hw, hw, 3), np.uint8)
for i in range(n):      # photo-like: smooth gradients, a few bars and a disc, light sensor noise
    im = np.repeat(base[..., None], 3, 2) + rng.integers(-3, 4, (hw, hw, 3))
    for k in range(6):
        t = int(rng.integers(50, hw - 50))
        im[t:t + 4, 40:hw - 40] += 90
        im[40:hw - 40, t:t + 4] -= 60
    cy, cx, r = rng.integers(200, hw - 200, 2).tolist() + [int(rng.integers(60, 180))]
    im[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] += 70
    photo[i] = np.clip(im, 0, 255)
noise = synthetic_images(3, n, hw, hw)[..., ::-1].copy()
say(f"fe_subject_region, {n} x {hw}x{hw}")
for name, batch in (("photo-like", photo), ("noise", noise)):
    rec, edges, thr = e.subject_contours(batch, want_edges=True, want_thresholds=True)
    comps = np.mean([len(r) for r in rec])
    t_all = timed(lambda: e.subject_contours(batch))
    d = e.dev_alloc(batch.nbytes)
    try:
        e.h2d(d, batch)
        t_res = timed(lambda: e.subject_contours((d, n, hw, hw)))
        t_stats = timed(lambda: e.image_stats((d, n, hw, hw)))
        t_lines = timed(lambda: e.leading_lines((d, n, hw, hw)), reps=1)
    finally:
        e.dev_free(d)
    t_cont = timed(lambda: e.external_contours(edges, min_twice_area=(hw * hw + 4999) // 5000))
    say(f"{name}: edge px/img {edges.astype(bool).sum() / n:.0f}  reported contours/img {comps:.1f}")
    say(f"   whole call, host input      {t_all * 1e3:9.1f} ms  {n / t_all:8.1f} images/s")
    say(f"   whole call, resident input  {t_res * 1e3:9.1f} ms  {n / t_res:8.1f} images/s")
    say(f"   gray + histogram alone      {t_stats * 1e3:9.1f} ms   (fe_image_stats, resident)")
    say(f"   labelling + external + walk {t_cont * 1e3:9.1f} ms   (fe_external_contours on the edge image, host input: includes its upload)")
    say(f"   Sobel + NMS + hysteresis    {max(0.0, t_res - t_stats - t_cont) * 1e3:9.1f} ms   (the rest of the resident call, by difference)")
    say(f"   fe_leading_lines, resident  {t_lines * 1e3:9.1f} ms   (for scale)")
for mid, nm in ((FE_MODEL_TOPIQ, "topiq"), (FE_MODEL_CLIP, "clip"), (FE_MODEL_AESTHETIC, "aesthetic"), (FE_MODEL_U2NETP, "u2netp"), (FE_MODEL_SAMP, "samp_net")):
    e.load_weights(mid, synthetic_state_dict(nm, 4))
rgb = photo[..., ::-1].copy()
t_off = timed(lambda: BatchScorer(e).process_batch(rgb), reps=2)
t_on = timed(lambda: BatchScorer(e, subject_region=True).process_batch(rgb), reps=2)
say(f"BatchScorer step, {n} photo-like images: subject_region off {t_off * 1e3:.1f} ms, on {t_on * 1e3:.1f} ms")
e.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines_out) + "\n")
