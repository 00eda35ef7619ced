"""BatchScorer.process_images on a chunk of 256 photos of about 1024 x 1024 spread over 1, 2, 16 and 256 distinct shapes, with
mixed_sizes off (one process_batch and one fe_ensemble_score per distinct shape: the path before the option existed, the baseline) and on
(one upload and one fe_ensemble_score_mixed per chunk), under the fp32 and parity policies, with the ensemble mask at 7 and at 6
(TOPIQ deselected: the reference's single-pass mode). Prints images/s and the device memory in use before the first and after the
first and the last chunk of a row. Rows of 1, 2 and 16 shapes repeat their chunk (the second run is timed); the row of 256 shapes runs
three chunks of 256 shapes each that no earlier chunk had (the last is timed), which is what a library of distinct sizes does to the
per-size tables. usage: perf_mixed.py [n] [chunks_of_256]     (written to profiles/mixed_sizes_perf.txt)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from facet_amd import Engine
from facet_amd._lib import FE_MODEL_AESTHETIC
from facet_amd.batch import BatchScorer
from facet_amd.precision import describe, load_models
from facet_amd.weights import synthetic_state_dict

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
fresh_chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
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


sds = {m: synthetic_state_dict(m, 4) for m in ("topiq", "clip", "u2netp", "samp_net")}
aes = synthetic_state_dict("aesthetic", 4)
print(f"{n} images per chunk, sides 776 .. 1280; images/s of process_images (upload included); device MiB in use: before / after first chunk / after last chunk")
print(f"{'policy':8} {'mask':>4} {'shapes':>6} {'mixed_sizes':>11} {'images/s':>9} {'MiB before':>11} {'first':>9} {'last':>9}")
for policy in ("f32", "parity"):
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
            for mixed in (False, True):
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
