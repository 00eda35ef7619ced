"""BatchScorer.process_images on a chunk of 256 photos of about 1024 x 1024 spread over 1, 2, 16 and 256 distinct shapes, with
mixed_sizes off (one process_batch and one fe_ensemble_score per distinct shape: the path before the option existed, the baseline) and on
(one upload and one fe_ensemble_score_mixed per chunk), under the fp32 and parity policies, with the ensemble mask at 7 and at 6
(TOPIQ deselected: the reference's single-pass mode). Prints images/s and the device memory in use before the first and after the
first and the last chunk of a row. Rows of 1, 2 and 16 shapes repeat their chunk (the second run is timed); the row of 256 shapes runs
three chunks of 256 shapes each that no earlier chunk had (the last is timed), which is what a library of distinct sizes does to the
per-size tables. usage: perf_mixed.py [n] [chunks_of_256] [--mixed-only] [--policies f32,parity]     (written to profiles/mixed_sizes_perf.txt)

perf_mixed.py --stats [--repeats R]: the technical statistics alone (written to profiles/mixed_stats_perf.txt). For the same chunk over 1, 16
and 256 shapes, resident as RGB: the per-shape-group path as process_batch does it (per group a device allocation, fe_swap_rb_u8,
fe_image_stats on the BGR copy, the frees), fe_image_stats alone on a BGR copy made beforehand, and one fe_image_stats_mixed call on the
RGB pixels at the default segment size and at 65 536, 262 144 and 1 048 576 pixels; then one 6000 x 4000 image alone. Every figure is
the median of R calls after one warm-up call, with the fastest and the slowest beside it.

perf_mixed.py --index [--repeats R]: the `phash` and `thumbnail` columns alone (written to profiles/mixed_index_perf.txt). The same chunks and
the 6000 x 4000 image: per shape group as process_batch computes them (a device allocation, fe_swap_rb_u8, fe_phash / fe_thumbnail_jpeg on
the BGR copy, the free - what a mixed chunk cost before fe_phash_mixed / fe_thumbnail_jpeg_mixed existed) against one mixed call on the RGB
pixels; then process_images with both columns on and mixed_sizes off / on, and the device memory in use over three chunks of new shapes.

perf_mixed.py --faces [--repeats R] [--det-thresh T]: the face stage alone (written to profiles/mixed_faces_perf.txt), with the stand-in
graphs of standins/ at det_size 640 and at most 8 faces kept per photo. The same chunks: per shape group as process_batch does it (a device
allocation, fe_swap_rb_u8, fe_face_analyze and fe_roi_laplacian on the BGR copy, the free) against one fe_face_analyze_mixed and one
fe_roi_laplacian_mixed call on the RGB pixels; then process_images with a face analyzer (gpu_thumbnails) on and mixed_sizes off / on, and
Engine.face_cache_entries() with the device memory in use over three chunks of new shapes. On a checkout without the mixed face calls only
the process_images rows and the per-shape memory row are printed: that is how the parent commit is measured in the same session.

perf_mixed.py --composition [--repeats R]: leading lines and the subject region alone (written to profiles/mixed_composition_perf.txt). The
same chunks and the 6000 x 4000 image, lines and subject separately: per shape group as process_batch does it (a device allocation,
fe_swap_rb_u8, fe_leading_lines / fe_subject_region on the BGR copy, the free) against one fe_leading_lines_mixed / fe_subject_region_mixed
call on the RGB pixels; for the lines also the milliseconds of the host stage (hysteresis + Hough on host threads, fe_lines_host_ms) inside
the median call. Then process_images with both options on (TOPIQ only) and mixed_sizes off / on, and the device memory in use over three
chunks of new shapes. On a checkout without the mixed calls only the process_images rows and the per-shape memory row are printed: that
is how the parent commit is measured in the same session."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from facet_amd import Engine
from facet_amd._lib import FE_MODEL_AESTHETIC, FE_MODEL_TOPIQ
from facet_amd.batch import BatchScorer
from facet_amd.precision import describe, load_models
from facet_amd.weights import synthetic_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=256)
ap.add_argument("chunks_of_256", nargs="?", type=int, default=3)
ap.add_argument("--mixed-only", action="store_true", help="skip the rows with mixed_sizes off")
ap.add_argument("--policies", default="f32,parity")
ap.add_argument("--stats", action="store_true", help="the statistics table instead of the process_images table")
ap.add_argument("--index", action="store_true", help="the pHash / thumbnail table instead of the process_images table")
ap.add_argument("--faces", action="store_true", help="the face-stage table instead of the process_images table")
ap.add_argument("--composition", action="store_true", help="the leading-lines / subject-region table instead of the process_images table")
ap.add_argument("--det-thresh", type=float, default=0.54, help="--faces: the stand-in detector's scores crowd around 0.5; 0.54 leaves a few faces per photo")
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
n, fresh_chunks = args.n, args.chunks_of_256
rng = np.random.default_rng(3)
yy, xx = np.mgrid[:1400, :1400].astype(np.float32)
field = np.clip(np.stack([120 + 70 * np.sin(xx / (40.0 + 9 * c)) * np.cos(yy / (55.0 - 7 * c)) for c in range(3)], -1)
                + rng.normal(0, 12, (1400, 1400, 3)), 0, 255).astype(np.uint8)


def shape(k):
    """Distinct for distinct k in 0 .. 4095: sides in 776 .. 1280, some past TOPIQ's 1024 cap."""
    return 776 + 8 * (k % 64), 1280 - 8 * (k // 64)


def chunk(shapes, first=0):
    """n windows of the field, image i with shape shapes[i % len(shapes)] (interleaved, as a folder lists them)."""
    out = []
    for i in range(n):
        h, w = shapes[i % len(shapes)]
        y, x = (37 * (first + i)) % (1400 - h + 1), (53 * (first + i)) % (1400 - w + 1)
        out.append(np.ascontiguousarray(field[y:y + h, x:x + w]))
    return out


def used_mib():
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 2**20


def timed(call, repeats):
    """Milliseconds of `call` (which returns after the engine stream has drained): median, fastest, slowest of `repeats` after one warm-up."""
    call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return f"{np.median(ts):9.2f} ({min(ts):.2f} .. {max(ts):.2f})"


def stats_rows(e, label, imgs, repeats):
    """imgs go up once, grouped by shape as _process_images_mixed lays them out; every path reads the resident RGB pixels."""
    groups = {}
    for i, a in enumerate(imgs):
        groups.setdefault(a.shape[:2], []).append(i)
    bufs, ptrs, sizes = [], [None] * len(imgs), [a.shape[:2] for a in imgs]
    for (h, w), idx in groups.items():
        d = e.dev_alloc(len(idx) * h * w * 3)
        e.h2d(d, np.stack([imgs[i] for i in idx]))
        bufs.append((d, len(idx), h, w))
        for j, i in enumerate(idx):
            ptrs[i] = d.value + j * h * w * 3

    def per_group():
        for d, k, h, w in bufs:
            d_bgr = e.dev_alloc(k * h * w * 3)
            try:
                e.swap_rb(d, k * h * w, d_bgr)
                e.image_stats((d_bgr, k, h, w))
            finally:
                e.dev_free(d_bgr)

    print(f"{label:22} {'per group: alloc + swap + fe_image_stats':42} {timed(per_group, repeats)}", flush=True)
    bgr = []
    for d, k, h, w in bufs:
        d_bgr = e.dev_alloc(k * h * w * 3)
        e.swap_rb(d, k * h * w, d_bgr)
        bgr.append((d_bgr, k, h, w))
    print(f"{label:22} {'per group: fe_image_stats alone (BGR ready)':42} {timed(lambda: [e.image_stats(b) for b in bgr], repeats)}", flush=True)
    for b in bgr:
        e.dev_free(b[0])
    for seg in (0, 65536, 262144, 1048576):
        e.set_stats_segment(seg)
        what = f"fe_image_stats_mixed, segment {seg if seg else 'default'}"
        print(f"{label:22} {what:42} {timed(lambda: e.image_stats_mixed((ptrs, sizes), order='rgb'), repeats)}", flush=True)
    e.set_stats_segment(0)
    for b in bufs:
        e.dev_free(b[0])


if args.stats:
    e = Engine(0, arena_bytes=4 << 30)
    print(f"{n} images per chunk, sides 776 .. 1280, resident RGB; milliseconds per chunk: median (fastest .. slowest) of {args.repeats} calls after a warm-up")
    for n_shapes in (1, 16, 256):
        shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
        stats_rows(e, f"{n} images, {n_shapes} shapes", chunk(shapes), args.repeats)
    stats_rows(e, "1 image 4000 x 6000", [np.ascontiguousarray(np.tile(field, (3, 5, 1))[:4000, :6000])], args.repeats)
    e.close()
    sys.exit(0)

def index_rows(e, label, imgs, repeats):
    """The two index columns of a chunk that is resident as RGB, grouped by shape as _process_images_mixed lays it out: per shape group as
    process_batch computes them (a device allocation, fe_swap_rb_u8, fe_phash / fe_thumbnail_jpeg on the BGR copy, the free) against one
    fe_phash_mixed / fe_thumbnail_jpeg_mixed call on the RGB pixels."""
    from facet_amd.phash import phash_batch, phash_mixed
    from facet_amd.thumbnail import thumbnails, thumbnails_mixed
    groups = {}
    for i, a in enumerate(imgs):
        groups.setdefault(a.shape[:2], []).append(i)
    bufs, ptrs, sizes = [], [None] * len(imgs), [a.shape[:2] for a in imgs]
    for (h, w), idx in groups.items():
        d = e.dev_alloc(len(idx) * h * w * 3)
        e.h2d(d, np.stack([imgs[i] for i in idx]))
        bufs.append((d, len(idx), h, w))
        for j, i in enumerate(idx):
            ptrs[i] = d.value + j * h * w * 3

    def per_group(stage):
        for d, k, h, w in bufs:
            d_bgr = e.dev_alloc(k * h * w * 3)
            try:
                e.swap_rb(d, k * h * w, d_bgr)
                stage((d_bgr, k, h, w))
            finally:
                e.dev_free(d_bgr)

    rows = (("phash", lambda b: phash_batch(e, b, bgr=True), lambda: phash_mixed(e, (ptrs, sizes))),
            ("thumbnail 640 q80", lambda b: thumbnails(e, b, 640, 80, bgr=True), lambda: thumbnails_mixed(e, (ptrs, sizes), 640, 80)))
    for name, stage, mixed in rows:
        print(f"{label:22} {name + ': per group (alloc + swap + call)':48} {timed(lambda: per_group(stage), repeats)}", flush=True)
        print(f"{label:22} {name + ': one mixed call':48} {timed(mixed, repeats)}", flush=True)
    for b in bufs:
        e.dev_free(b[0])


if args.index:
    e = Engine(0, arena_bytes=(4 + 2 * 8) << 30)      # bench.py's arena for the default micro-batch of 8 at 1024 x 1024
    print(f"{n} images per chunk, sides 776 .. 1280, resident RGB; milliseconds per chunk: median (fastest .. slowest) of {args.repeats} calls after a warm-up")
    for n_shapes in (1, 16, 256):
        shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
        index_rows(e, f"{n} images, {n_shapes} shapes", chunk(shapes), args.repeats)
    index_rows(e, "1 image 4000 x 6000", [np.ascontiguousarray(np.tile(field, (3, 5, 1))[:4000, :6000])], args.repeats)
    # process_images with both columns on (TOPIQ loaded, the other models left out): one process_batch per shape against the mixed path
    e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 4))
    print("process_images, phash + thumbnails on, TOPIQ only: milliseconds per chunk (upload included)")
    for n_shapes in (1, 16, 256):
        shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
        imgs = chunk(shapes)
        for mixed in (False, True):
            bs = BatchScorer(e, mixed_sizes=mixed, phash=True, thumbnails=True)
            print(f"{n} images, {n_shapes:3} shapes  mixed_sizes={str(mixed):5} {timed(lambda: bs.process_images(imgs), max(3, args.repeats // 2))}", flush=True)
    # device memory over three chunks of 256 shapes no earlier chunk had: the per-size tables of the per-group calls stay, the pools go
    print("device MiB in use before / after each of three chunks of new shapes (phash + thumbnail of every image)")
    from facet_amd.phash import phash_mixed
    from facet_amd.thumbnail import thumbnails, thumbnails_mixed
    next_shape = 1024
    for mixed in (False, True):
        mem = [used_mib()]
        for r in range(3):
            imgs = chunk([shape(next_shape + k) for k in range(256)], first=r * n)
            next_shape += 256
            if mixed:
                phash_mixed(e, imgs); thumbnails_mixed(e, imgs, 640, 80)
            else:
                for a in imgs:
                    e.phash(a[None]); thumbnails(e, a[None], 640, 80)
            mem.append(used_mib())
        print(f"{'one mixed call each' if mixed else 'per shape':22} tables {e.resize_cache_entries():5}  MiB " + " / ".join(f"{m:.0f}" for m in mem), flush=True)
    e.close()
    sys.exit(0)

FACE_DET, FACE_NMS, FACE_MAX = (640, 640), 0.4, 8


def face_rois(rec, counts, sizes):
    """The face boxes a call found, clipped to their images as FaceAnalyzer._get_crop_sharpness clips them: (image indices, rois)."""
    idx, rois = [], []
    for i, (h, w) in enumerate(sizes):
        for f in range(min(int(counts[i]), rec.shape[1])):
            x1, y1, x2, y2 = (int(v) for v in rec[i, f, 0:4])
            x1, y1, x2, y2 = max(0, x1), max(0, y1), min(w, x2), min(h, y2)
            if x2 > x1 and y2 > y1:
                idx.append(i); rois.append((x1, y1, x2, y2))
    return idx, rois


def face_rows(e, label, imgs, repeats):
    """The face stage of a chunk that is resident as RGB, grouped by shape as _process_images_mixed lays it out."""
    groups = {}
    for i, a in enumerate(imgs):
        groups.setdefault(a.shape[:2], []).append(i)
    bufs, ptrs, sizes = [], [None] * len(imgs), [a.shape[:2] for a in imgs]
    for (h, w), idx in groups.items():
        d = e.dev_alloc(len(idx) * h * w * 3)
        e.h2d(d, np.stack([imgs[i] for i in idx]))
        bufs.append((d, len(idx), h, w))
        for j, i in enumerate(idx):
            ptrs[i] = d.value + j * h * w * 3
    found, kept = [0, 0], [0, 0]      # ROIs scanned and faces kept (they went through the two crop graphs): per group, mixed

    def per_group():
        found[0] = kept[0] = 0
        for d, k, h, w in bufs:
            d_bgr = e.dev_alloc(k * h * w * 3)
            try:
                e.swap_rb(d, k * h * w, d_bgr)
                rec, counts, _ = e.face_analyze((d_bgr, k, h, w), FACE_DET, args.det_thresh, FACE_NMS, FACE_MAX)
                idx, rois = face_rois(rec, counts, [(h, w)] * k)
                found[0] += len(idx)
                kept[0] += int(np.minimum(counts, FACE_MAX).sum())
                if idx:
                    e.roi_laplacian((d_bgr, k, h, w), idx, rois)
            finally:
                e.dev_free(d_bgr)

    def mixed():
        rec, counts, _ = e.face_analyze_mixed((ptrs, sizes), FACE_DET, args.det_thresh, FACE_NMS, FACE_MAX, order='rgb')
        idx, rois = face_rois(rec, counts, sizes)
        found[1], kept[1] = len(idx), int(np.minimum(counts, FACE_MAX).sum())
        if idx:
            e.roi_laplacian_mixed((ptrs, sizes), idx, rois, order='rgb')

    print(f"{label:22} {'per group: alloc + swap + fe_face_analyze + fe_roi_laplacian':62} {timed(per_group, repeats)}", flush=True)
    print(f"{label:22} {'fe_face_analyze_mixed + fe_roi_laplacian_mixed':62} {timed(mixed, repeats)}", flush=True)
    what = 'fe_face_analyze_mixed alone'
    print(f"{label:22} {what:62} {timed(lambda: e.face_analyze_mixed((ptrs, sizes), FACE_DET, args.det_thresh, FACE_NMS, FACE_MAX, order='rgb'), repeats)}", flush=True)
    print(f"{label:22} faces kept (landmark and recognition crops): {kept[0]} per group, {kept[1]} mixed; ROIs scanned: {found[0]}, {found[1]}", flush=True)
    for b in bufs:
        e.dev_free(b[0])


if args.faces:
    from standins import synthetic_onnx as S
    from facet_amd.face import FaceAnalyzer
    has_mixed = hasattr(Engine, "face_analyze_mixed")
    e = Engine(0, arena_bytes=(4 + 2 * 8) << 30)      # bench.py's arena for the default micro-batch of 8 at 1024 x 1024
    models = {"det": S.scrfd_like(seed=12, size=640)[0], "lmk": S.landmark_like(seed=13)[0], "rec": S.arcface_iresnet(layers=(1, 1, 1, 1), seed=14)[0]}
    fa = FaceAnalyzer(min_confidence=args.det_thresh, min_face_size=10, engine=e, models=models, gpu_thumbnails=True)
    assert fa.available
    fa.face_app.det_thresh, fa.face_app.max_candidates, fa.face_app.max_faces = args.det_thresh, 4096, FACE_MAX
    print(f"{n} images per chunk, sides 776 .. 1280, resident RGB; stand-in graphs, det_size 640, det_thresh {args.det_thresh}, at most {FACE_MAX} faces kept per image")
    print(f"milliseconds per chunk: median (fastest .. slowest) of {args.repeats} calls after a warm-up")
    if has_mixed:
        for n_shapes in (1, 16, 256):
            shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
            face_rows(e, f"{n} images, {n_shapes} shapes", chunk(shapes), args.repeats)
    e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 4))
    print("process_images, face analyzer (gpu_thumbnails) on, TOPIQ only: milliseconds per chunk (upload included)")
    for n_shapes in (1, 16, 256):
        shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
        imgs = chunk(shapes)
        for mixed in (False, True):
            bs = BatchScorer(e, face_analyzer=fa, mixed_sizes=mixed)
            print(f"{n} images, {n_shapes:3} shapes  mixed_sizes={str(mixed):5} {timed(lambda: bs.process_images(imgs), max(3, args.repeats // 2))}", flush=True)
    print("cv2.resize tables kept by the context and device MiB in use before / after each of three chunks of new shapes (faces of every image)")
    next_shape = 1024
    for mixed in ((False, True) if has_mixed else (False,)):
        mem = [used_mib()]
        tables = [e.face_cache_entries()] if has_mixed else []
        for r in range(3):
            imgs = chunk([shape(next_shape + k) for k in range(256)], first=r * n)
            next_shape += 256
            if mixed:
                e.face_analyze_mixed(imgs, FACE_DET, args.det_thresh, FACE_NMS, FACE_MAX, order='rgb')
            else:
                for a in imgs:
                    e.face_analyze(a[None], FACE_DET, args.det_thresh, FACE_NMS, FACE_MAX)
            mem.append(used_mib())
            if has_mixed:
                tables.append(e.face_cache_entries())
        print(f"{'one mixed call' if mixed else 'per shape':22} " + ("tables " + " / ".join(str(t) for t in tables) + "  " if has_mixed else "") +
              "MiB " + " / ".join(f"{m:.0f}" for m in mem), flush=True)
    e.close()
    sys.exit(0)

def composition_rows(e, label, imgs, repeats):
    """Lines and subject region of a chunk that is resident as RGB, grouped by shape as _process_images_mixed lays it out: per shape group
    as process_batch computes them against one mixed call on the RGB pixels."""
    groups = {}
    for i, a in enumerate(imgs):
        groups.setdefault(a.shape[:2], []).append(i)
    bufs, ptrs, sizes = [], [None] * len(imgs), [a.shape[:2] for a in imgs]
    for (h, w), idx in groups.items():
        d = e.dev_alloc(len(idx) * h * w * 3)
        e.h2d(d, np.stack([imgs[i] for i in idx]))
        bufs.append((d, len(idx), h, w))
        for j, i in enumerate(idx):
            ptrs[i] = d.value + j * h * w * 3
    host = []

    def per_group(stage, lines):
        ms = 0.0
        for d, k, h, w in bufs:
            d_bgr = e.dev_alloc(k * h * w * 3)
            try:
                e.swap_rb(d, k * h * w, d_bgr)
                stage((d_bgr, k, h, w))
                ms += e.lines_host_ms() if lines else 0.0
            finally:
                e.dev_free(d_bgr)
        host.append(ms)

    def mixed_lines():
        e.leading_lines_mixed((ptrs, sizes), order='rgb')
        host.append(e.lines_host_ms())

    rows = (("lines", lambda: per_group(e.leading_lines, True), mixed_lines),
            ("subject", lambda: per_group(e.subject_contours, False), lambda: e.subject_contours_mixed((ptrs, sizes), order='rgb')))
    for name, grouped, mixed in rows:
        for what, call in ((name + ": per group (alloc + swap + call)", grouped), (name + ": one mixed call", mixed)):
            del host[:]
            t = timed(call, repeats)
            stage = f"   host stage {np.median(host[1:]):9.2f}" if name == "lines" else ""
            print(f"{label:22} {what:44} {t}{stage}", flush=True)
    for b in bufs:
        e.dev_free(b[0])


if args.composition:
    has_mixed = hasattr(Engine, "leading_lines_mixed")
    e = Engine(0, arena_bytes=(4 + 2 * 8) << 30)      # bench.py's arena for the default micro-batch of 8 at 1024 x 1024
    print(f"{n} images per chunk, sides 776 .. 1280, resident RGB; milliseconds per chunk: median (fastest .. slowest) of {args.repeats} calls after a warm-up")
    if has_mixed:
        for n_shapes in (1, 16, 256):
            shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
            composition_rows(e, f"{n} images, {n_shapes} shapes", chunk(shapes), args.repeats)
        composition_rows(e, "1 image 4000 x 6000", [np.ascontiguousarray(np.tile(field, (3, 5, 1))[:4000, :6000])], args.repeats)
    e.load_weights(FE_MODEL_TOPIQ, synthetic_state_dict("topiq", 4))
    print("process_images, detect_lines + subject_region on, TOPIQ only: milliseconds per chunk (upload included)")
    for n_shapes in (1, 16, 256):
        shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
        imgs = chunk(shapes)
        for mixed in (False, True):
            bs = BatchScorer(e, mixed_sizes=mixed, detect_lines=True, subject_region=True)
            print(f"{n} images, {n_shapes:3} shapes  mixed_sizes={str(mixed):5} {timed(lambda: bs.process_images(imgs), max(3, args.repeats // 2))}", flush=True)
    print("device MiB in use before / after each of three chunks of new shapes (lines + subject region of every image)")
    next_shape = 1024
    for mixed in ((False, True) if has_mixed else (False,)):
        mem = [used_mib()]
        for r in range(3):
            imgs = chunk([shape(next_shape + k) for k in range(256)], first=r * n)
            next_shape += 256
            if mixed:
                e.leading_lines_mixed(imgs, order='rgb'); e.subject_contours_mixed(imgs, order='rgb')
            else:
                for a in imgs:
                    e.leading_lines(a[None]); e.subject_contours(a[None])
            mem.append(used_mib())
        print(f"{'one mixed call each' if mixed else 'per shape':22} MiB " + " / ".join(f"{m:.0f}" for m in mem), flush=True)
    e.close()
    sys.exit(0)

sds = {m: synthetic_state_dict(m, 4) for m in ("topiq", "clip", "u2netp", "samp_net")}
aes = synthetic_state_dict("aesthetic", 4)
print(f"{n} images per chunk, sides 776 .. 1280; images/s of process_images (upload included); device MiB in use: before / after first chunk / after last chunk")
print(f"{'policy':8} {'mask':>4} {'shapes':>6} {'mixed_sizes':>11} {'images/s':>9} {'MiB before':>11} {'first':>9} {'last':>9}")
for policy in args.policies.split(","):
    e = Engine(0, arena_bytes=(4 + 2 * 32) << 30)      # bench.py's arena for micro-batch 32 at 1024 x 1024
    load_models(e, policy, sds)
    e.load_weights(FE_MODEL_AESTHETIC, aes)
    e.set_microbatch(32)
    print(f"# {policy}: {describe(policy)}", flush=True)
    BatchScorer(e).process_images(chunk([(1024, 1024)])[:8])      # buffers of the first call
    next_shape = 0
    for mask in (7, 6):
        e.ensemble_select(mask)
        for n_shapes in (1, 2, 16, 256):
            for mixed in ((True,) if args.mixed_only else (False, True)):
                bs = BatchScorer(e, mixed_sizes=mixed)
                before = used_mib()
                runs = fresh_chunks if n_shapes == 256 else 2
                after = []
                for r in range(runs):
                    if n_shapes == 256:      # shapes no earlier chunk of this context had
                        shapes = [shape(next_shape + k) for k in range(n_shapes)]
                        next_shape += n_shapes
                    else:
                        shapes = [shape(17 * k + 5) for k in range(n_shapes)] if n_shapes > 1 else [(1024, 1024)]
                    imgs = chunk(shapes, first=r * n)
                    t0 = time.time()
                    out = bs.process_images(imgs)
                    dt = time.time() - t0
                    assert len(out) == n and all(o is not None for o in out)
                    after.append(used_mib())
                print(f"{policy:8} {mask:>4} {n_shapes:>6} {str(mixed):>11} {n / dt:>9.1f} {before:>11.0f} {after[0]:>9.0f} {after[-1]:>9.0f}", flush=True)
    e.close()
