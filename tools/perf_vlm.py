"""Throughput of the VLM tagger's text decoder at Qwen2.5-VL-7B's geometry (BASELINE configs[4] shape; slice 1 = decoder only).

  python tools/perf_vlm.py [--layers 28] [--prompt 512] [--new 32] [--batches 1,8,32] [--vision N] [--from-rgb N] [--pad P]
  python tools/perf_vlm.py --family qwen3 [--prompt 512] [--new 32] [--batches 1,4,32] [--vision N]
  python tools/perf_vlm.py --scores [--layers 4] [--prompt 512] [--new 32] [--batches 1,4,32] [--reps 7]
  python tools/perf_vlm.py --weights bf16,fp8 [--kv bf16,fp8] [--family qwen2_5|qwen3|qwen2] [--layers 8] [--prompt 512] [--new 32] [--batches 1,4,32] [--reps 5]

--weights: one column per weight format (Engine.vlm_weight_format) of the chosen family's decoder - qwen3 / qwen2 at full depth, qwen2_5 at
--layers layers of the 7B geometry. Every format's engine is loaded with the same seeded weights; the formats are timed alternately,
--reps times each, per batch: prefill tokens/s (device timer) and the device-resident decode loop (fe_vlm_generate; host clock around the
call, which ends in a synchronise) as median ms/step with the spread of the repetitions, tokens/s, and the fraction of the 8 TB/s HBM peak
that the bytes of fe_vlm_weight_info (weights + row scales, streamed once per step) amount to at that time.

--kv: crossed with --weights (bf16 alone when that is not given), one column per (weight format, KV-cache format) pair
(Engine.vlm_kv_format: bf16, fp8, bf16_e4m3); the pairs are timed alternately like the weight formats. Each row also gives the K / V bytes
a decode step reads at the middle of the call (fe_vlm_kv_info's bytes per token x sequences x cached tokens) beside the weight bytes; the
HBM fraction is of their sum.

--scores: the device-resident decode loop with the chosen tokens' log-probs (fe_vlm_generate_scored) against the plain loop
(fe_vlm_generate) at the 7B geometry, same prefill, --reps alternating repetitions of each; prints the median ms/step of both and the
difference, and checks that the ids are identical.

--family qwen3: Qwen3-VL-2B at full depth (28 decoder layers of hidden 2048, 16 / 8 heads of 128, intermediate 6144, tied vocab 151936;
tower of 24 blocks of 1024, 16 heads of 64, DeepStack after 5 / 11 / 17), ~4 GB of seeded synthetic weights, no extrapolation: prefill
tokens/s, decode ms/step and the fraction of HBM peak of the weight stream, the Qwen2.5-VL decoder at --qwen25-layers layers at batch 4 in
the same run for comparison, and the vision tower's images/s at the max_pixels grid (480 x 768 -> 30 x 48 patches) with inputs resident.

--from-rgb N times the vision tower from N uint8 photos (GPU preprocessing: fe_vlm_preprocess_rgb + fe_vlm_encode_preprocessed) against
the same photos' fp32 pixel_values uploaded by fe_vlm_encode_images; --pad P also times the decode steps of a left-padded batch (every
other sequence carries P pad tokens; fe_vlm_prefill_images_padded) next to the unpadded one.

Seeded synthetic weights in the 7B geometry (hidden 3584, 28 q heads over 4 KV heads of 128, intermediate 18944, vocab 152064); with
--layers < 28 the per-layer work is measured on that many layers and the lm_head once, and both the measured and the 28-layer
extrapolation are printed. Prefill is matrix-core bound (2 * parameters * tokens FLOPs); decode is HBM bound (every weight byte once per
step, whatever the batch) - the decode line reports GB/s of weight traffic against the 8 TB/s peak.
"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from facet_amd import Engine
from facet_amd._lib import FE_MODEL_VLM
from facet_amd.weights import synthetic_state_dict, qwen2_5_vl_text_spec

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--prompt", type=int, default=512)
ap.add_argument("--new", type=int, default=16)
ap.add_argument("--batches", default="1,8,32")
ap.add_argument("--vision", type=int, default=0, help="also time the vision tower: this many images of 1036x1036 pixels (74x74 patches) per call, full depth 32")
ap.add_argument("--from-rgb", type=int, default=0, help="time vision encode from this many uint8 1036x1036 photos against the fp32 pixel_values upload")
ap.add_argument("--pad", type=int, default=0, help="also time decode steps with every other sequence left-padded by this many tokens")
ap.add_argument("--family", default="qwen2_5", choices=("qwen2_5", "qwen3", "qwen2"))
ap.add_argument("--qwen25-layers", type=int, default=4, help="--family qwen3: layers of the Qwen2.5-VL-7B decoder timed at batch 4 for comparison")
ap.add_argument("--scores", action="store_true", help="time fe_vlm_generate_scored against fe_vlm_generate (ms/step) and stop")
ap.add_argument("--reps", type=int, default=7, help="--scores / --weights: alternating repetitions of each loop")
ap.add_argument("--weights", default=None, help="comma-separated weight formats (bf16, fp8): one column per format, then stop")
ap.add_argument("--kv", default=None, help="comma-separated KV-cache formats (bf16, fp8, bf16_e4m3), crossed with --weights")
a = ap.parse_args()


def decode_rate(e, B, L, new, V):
    """(prefill ms, decode ms/step through fe_vlm_decode_step, device-resident ms/step through fe_vlm_generate) of B random prompts of L."""
    p = np.random.default_rng(B).integers(0, V, (B, L)).astype(np.int32)
    e.vlm_prefill(p, max_seq=L + new + 8)
    e.timer_start(); nxt = e.vlm_prefill(p, max_seq=L + new + 8); t_pre = e.timer_stop()
    pos = np.full((3, B), L, np.int32)
    e.vlm_decode_step(nxt, pos)
    t0 = time.perf_counter()
    for s in range(new):
        nxt = e.vlm_decode_step(nxt, pos + 1 + s)
    t_dec = (time.perf_counter() - t0) / new * 1e3
    e.vlm_prefill(p, max_seq=L + new + 8)
    t0 = time.perf_counter(); e.vlm_generate(p, new + 1); t_all = (time.perf_counter() - t0) * 1e3
    return t_pre, t_dec, (t_all - t_pre) / new


def weights_table():
    from facet_amd.weights import qwen2_vl_text_spec, qwen3_vl_text_spec
    from facet_amd.vlm_composition import QWEN2_VL_2B
    from facet_amd.vlm_tagger import QWEN3_VL_2B
    fmts = (a.weights or "bf16").split(",")
    kvs = a.kv.split(",") if a.kv else [None]
    cols = [(f, kv) for f in fmts for kv in kvs]
    name = lambda c: c[0] if c[1] is None else f"{c[0]}/kv-{c[1]}"
    if a.family == "qwen3":
        spec, V, what = qwen3_vl_text_spec(), 151936, "Qwen3-VL-2B decoder, 28 layers (full depth), tied head"
        conf = lambda e: e.vlm3_configure(**QWEN3_VL_2B)
    elif a.family == "qwen2":
        spec, V, what = qwen2_vl_text_spec(), 151936, "Qwen2-VL-2B decoder, 28 layers (full depth), tied head"
        conf = lambda e: e.vlm2_configure(**QWEN2_VL_2B)
    else:
        spec, V = qwen2_5_vl_text_spec(hidden=3584, layers=a.layers, heads=28, kv_heads=4, inter=18944, vocab=152064), 152064
        what = f"Qwen2.5-VL-7B decoder geometry, {a.layers} of 28 layers + lm_head"
        conf = lambda e: e.vlm_configure(28, 4, 128, 1e6, 1e-6, (16, 24, 24))
    sd = synthetic_state_dict(None, 3, spec=spec)
    eng, info = {}, {}
    for c in cols:                                       # one engine per column: no column pays for another's cache or scratch
        e = Engine(0, arena_bytes=24 << 30)
        conf(e)
        e.vlm_weight_format(c[0])
        if c[1] is not None:
            e.vlm_kv_format(c[1])
        t0 = time.time(); e.load_weights(FE_MODEL_VLM, sd)
        eng[c], info[c] = e, e.vlm_weight_info()
        print(f"{name(c)}: committed in {time.time() - t0:.0f} s: {info[c]}", flush=True)
    del sd
    L, new = a.prompt, a.new
    print(f"{what}; prompt {L}, {new} decode steps per call, median (min..max) of {a.reps} alternating calls per format", flush=True)
    for B in [int(b) for b in a.batches.split(",")]:
        p = np.random.default_rng(B).integers(0, V, (B, L)).astype(np.int32)
        pre, dec, kvinfo = {c: [] for c in cols}, {c: [] for c in cols}, {}
        for r in range(a.reps + 1):                      # (the first round warms up: graph capture, first-use attributes)
            for c in cols:
                e = eng[c]
                e.timer_start(); e.vlm_prefill(p, max_seq=L + new + 8); t_pre = e.timer_stop()
                e.sync()
                t0 = time.perf_counter(); e.vlm_generate(p, new + 1); t_all = (time.perf_counter() - t0) * 1e3
                if c[1] is not None:
                    kvinfo[c] = e.vlm_kv_info()
                if r:
                    pre[c].append(t_pre); dec[c].append((t_all - t_pre) / new)
        for c in cols:
            t, tp = float(np.median(dec[c])), float(np.median(pre[c]))
            by = info[c]["weight_bytes"] + info[c]["scale_bytes"]
            kvtxt = ""
            if c[1] is not None:
                kvb = kvinfo[c]["bytes_per_token"] * B * (L + new // 2)
                kvtxt = f"weights + {kvb / 1e9:.3f} GB of K/V ({kvinfo[c]['bytes_per_token']} B per token, {kvinfo[c]['allocated_bytes'] / 1e9:.3f} GB allocated) = "
                by += kvb
            print(f"{a.family} {name(c):4s} B={B:3d}: prefill {B * L / tp * 1e3:9.0f} tok/s ({tp:.2f} ms) | decode {t:7.4f} ms/step ({min(dec[c]):.4f}..{max(dec[c]):.4f}) = "
                  f"{B / t * 1e3:8.0f} tok/s | {kvtxt}{by / 1e9:.3f} GB per step = {by / t / 1e6:6.0f} GB/s = {by / t / 1e6 / 8000:.3f} of HBM peak", flush=True)
        if len(cols) > 1:
            t0 = float(np.median(dec[cols[0]]))
            print("    decode ms/step " + ", ".join(f"{name(c)} / {name(cols[0])} = {float(np.median(dec[c])) / t0:.3f}" for c in cols[1:]), flush=True)
    for e in eng.values():
        e.close()


if a.weights or a.kv:
    weights_table()
    sys.exit(0)
if a.family == "qwen2":
    # Qwen2-VL-2B (the composition model) at full depth: tower at 1296 and 5120 patches, prefill, decode ms/step at the --batches, and the
    # stop-at-EOS loop against the full one at 256 steps when every row finishes by step 64. Every figure beside its HBM-bound estimate.
    from facet_amd.weights import qwen2_vl_text_spec, qwen2_vl_vision_spec
    from facet_amd.vlm_composition import QWEN2_VL_2B
    from facet_amd.vlm_tagger import vision_inputs_qwen2
    H, NH, NKV, INTER, V, NL = 1536, 12, 2, 8960, 151936, 28
    t0 = time.time()
    sd = synthetic_state_dict(None, 3, spec=qwen2_vl_text_spec() + qwen2_vl_vision_spec())
    print(f"weights drawn in {time.time() - t0:.0f} s ({sum(v.size for v in sd.values()) / 1e9:.2f} G parameters)", flush=True)
    e = Engine(0, arena_bytes=40 << 30)
    e.vlm2_configure(**QWEN2_VL_2B)
    t0 = time.time(); e.load_weights(FE_MODEL_VLM, sd); del sd
    print(f"committed in {time.time() - t0:.0f} s", flush=True)
    vis_params = 32 * (4 * 1280 * 1280 + 2 * 1280 * 5120) + 5120 * 5120 + 5120 * 1536 + 1176 * 1280
    for gh, gw in ((36, 36), (64, 80)):      # 1296 and 5120 patches
        v = vision_inputs_qwen2([[1, gh, gw]])
        n = gh * gw
        pv = np.random.default_rng(0).normal(0, 1, (n, 1176)).astype(np.float32)
        e.vlm2_encode_images(pv, v["patch_pos_hw"], v["cu_seqlens"], want_embeds=False)
        rgb = [np.random.default_rng(1).integers(0, 256, (gh * 14, gw * 14, 3), dtype=np.uint8)]
        e.vlm_preprocess_rgb(rgb, [(gh * 14, gw * 14)], (0.5,) * 3, (0.5,) * 3)
        e.vlm2_encode_images(None, v["patch_pos_hw"], v["cu_seqlens"], want_embeds=False)
        e.flops_reset(); e.timer_start()
        e.vlm2_encode_images(None, v["patch_pos_hw"], v["cu_seqlens"], want_embeds=False)
        ms = e.timer_stop()
        attn = 4.0 * 32 * n * n * 1280
        print(f"vision tower (qwen2, 32 blocks): {n} patches ({n // 4} image tokens), rows resident: {ms:.2f} ms, {e.flops() / ms / 1e9:.1f} TFLOP/s "
              f"(projections), attention {attn / 1e9:.0f} GFLOP more | weight stream {2 * vis_params / 1e9:.2f} GB = {2 * vis_params / 8e9:.3f} ms at HBM peak "
              f"(compute-bound: {(2.0 * n * vis_params + attn) / 2.5e12:.2f} ms at 2.5 PFLOP/s dense bf16)", flush=True)
    layer_params = H * (NH + 2 * NKV) * 128 + NH * 128 * H + 3 * H * INTER
    wbytes = 2.0 * (NL * layer_params + V * H)
    for B in [int(b) for b in a.batches.split(",")]:
        L = a.prompt
        t_pre, t_dec, t_loop = decode_rate(e, B, L, a.new, V)
        print(f"qwen2 B={B:3d} L={L}: prefill {t_pre:8.2f} ms = {B * L / t_pre * 1e3:9.0f} tok/s | decode {t_dec:6.3f} ms/step | device-resident loop "
              f"{t_loop:6.3f} ms/step = {wbytes / t_loop / 1e6:6.0f} GB/s = {wbytes / t_loop / 1e6 / 8000:.2f} of HBM peak (HBM-bound estimate "
              f"{wbytes / 8e9:.3f} ms/step: {wbytes / 1e9:.2f} GB of bf16 weights per step)", flush=True)
    # generate_until against generate: 256 steps, EOS ids = what each row emits at step 63 of the full run (every row finishes by step 64)
    B, L, STEPS = 8, a.prompt, 256
    p = np.random.default_rng(B).integers(0, V, (B, L)).astype(np.int32)
    pos = np.full((3, B), L, np.int32)
    first = e.vlm_prefill(p, max_seq=L + STEPS + 8)
    full, _, ran = e.vlm_generate_until(first, pos, STEPS, [], poll=8)
    assert ran == STEPS
    eos = sorted(set(int(t) for t in full[63]))[:8]
    import ctypes as C
    i32p = C.POINTER(C.c_int32)
    sink = np.empty((STEPS, B), np.int32)
    tg = 1e9      # the baseline: fe_vlm_generate, which never reads anything back between steps
    for _ in range(3):
        first = np.ascontiguousarray(e.vlm_prefill(p, max_seq=L + STEPS + 8), dtype=np.int32)
        t0 = time.perf_counter()
        e._ck(e.lib.fe_vlm_generate(e.h, first.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), B, STEPS, sink.ctypes.data_as(i32p)))
        tg = min(tg, (time.perf_counter() - t0) * 1e3)
    assert np.array_equal(sink, full)
    print(f"qwen2 B={B} fe_vlm_generate: {tg:.1f} ms for {STEPS} steps = {tg / STEPS:.3f} ms/step", flush=True)
    for poll in (8, 1):
        t = {}
        for name, ids in (("noeos", []), ("until", eos)):
            best = 1e9
            for _ in range(3):
                first = e.vlm_prefill(p, max_seq=L + STEPS + 8)
                t0 = time.perf_counter(); _, _, ran = e.vlm_generate_until(first, pos, STEPS, ids, poll=poll); best = min(best, (time.perf_counter() - t0) * 1e3)
            t[name] = (best, ran)
        (tn, rn), (tu, ru) = t["noeos"], t["until"]
        print(f"qwen2 B={B} generate_until poll={poll}: {tu:.1f} ms for {ru} steps: until / generate = {tu / tg:.3f} beside steps_run / {STEPS} = {ru / STEPS:.3f} "
              f"({tu / ru:.3f} vs {tg / STEPS:.3f} ms/step, {ru // poll} host reads of the running count) | all {rn} steps with the polls and no EOS id: "
              f"{tn:.1f} ms = {tn / tg:.3f} of generate: the poll syncs cost {(tn - tg) / max(1, rn // poll) * 1e3:.0f} us each", flush=True)
    e.close()
    sys.exit(0)
if a.family == "qwen3":
    from facet_amd.weights import qwen3_vl_text_spec, qwen3_vl_vision_spec
    from facet_amd.vlm_tagger import QWEN3_VL_2B, vision_inputs_qwen3
    H, NH, NKV, INTER, V, NL = 2048, 16, 8, 6144, 151936, 28
    t0 = time.time()
    spec = qwen3_vl_text_spec(hidden=H, layers=NL, heads=NH, kv_heads=NKV, inter=INTER, vocab=V) + (qwen3_vl_vision_spec() if a.vision else [])
    sd = synthetic_state_dict(None, 3, spec=spec)
    print(f"weights drawn in {time.time() - t0:.0f} s ({sum(v.size for v in sd.values()) / 1e9:.2f} G parameters)", flush=True)
    e = Engine(0, arena_bytes=40 << 30)
    e.vlm3_configure(**QWEN3_VL_2B)
    t0 = time.time(); e.load_weights(FE_MODEL_VLM, sd); del sd
    print(f"committed in {time.time() - t0:.0f} s", flush=True)
    if a.vision:
        g = [[1, 30, 48]] * a.vision                     # smart_resize(900, 1400, 32, 65536, 512*28*28) = 480 x 768
        v = vision_inputs_qwen3(g, 48)
        n = 30 * 48 * a.vision
        pv = np.random.default_rng(0).normal(0, 1, (n, 1536)).astype(np.float32)
        args = (v["patch_pos_hw"], v["interp_idx"], v["interp_w"], v["cu_seqlens"])
        e.vlm3_encode_images(pv, *args, want_embeds=False)
        # inputs resident: the bf16 rows of a preprocess stay on the device (pixel_values=None)
        rgb = [np.random.default_rng(i).integers(0, 256, (480, 768, 3), dtype=np.uint8) for i in range(a.vision)]
        e.vlm_preprocess_rgb(rgb, [(480, 768)] * a.vision, (0.5,) * 3, (0.5,) * 3)
        e.vlm3_encode_images(None, *args, want_embeds=False)
        e.flops_reset(); e.timer_start()
        e.vlm3_encode_images(None, *args, want_embeds=False)
        ms = e.timer_stop()
        print(f"vision tower (qwen3, 24 blocks): {a.vision} images of 30x48 patches (360 image tokens each), rows resident: {ms:.2f} ms = "
              f"{a.vision / ms * 1e3:.1f} images/s, {e.flops() / ms / 1e9:.1f} TFLOP/s (projections)", flush=True)
    layer_params = H * (NH + 2 * NKV) * 128 + NH * 128 * H + 3 * H * INTER
    wbytes = 2.0 * (NL * layer_params + V * H)
    for B in [int(b) for b in a.batches.split(",")]:
        L = a.prompt
        t_pre, t_dec, t_loop = decode_rate(e, B, L, a.new, V)
        print(f"qwen3 B={B:3d} L={L}: prefill {t_pre:8.2f} ms = {B * L / t_pre * 1e3:9.0f} tok/s | decode {t_dec:6.3f} ms/step = "
              f"{wbytes / t_dec / 1e6 / 8000:.2f} of HBM peak | device-resident loop {t_loop:6.3f} ms/step = {wbytes / t_loop / 1e6:6.0f} GB/s = "
              f"{wbytes / t_loop / 1e6 / 8000:.2f} of peak ({NL} layers, {wbytes / 1e9:.2f} GB of weights per step)", flush=True)
    e.close()
    if a.qwen25_layers > 0:      # the Qwen2.5-VL-7B decoder at batch 4 in the same process, for the HBM-fraction comparison
        H2, NH2, NKV2, I2, V2 = 3584, 28, 4, 18944, 152064
        sd = synthetic_state_dict(None, 3, spec=qwen2_5_vl_text_spec(hidden=H2, layers=a.qwen25_layers, heads=NH2, kv_heads=NKV2, inter=I2, vocab=V2))
        e = Engine(0, arena_bytes=40 << 30)
        e.vlm_configure(NH2, NKV2, 128, 1e6, 1e-6, (16, 24, 24))
        e.load_weights(FE_MODEL_VLM, sd); del sd
        lp2 = H2 * (NH2 + 2 * NKV2) * 128 + NH2 * 128 * H2 + 3 * H2 * I2
        wb2 = 2.0 * (a.qwen25_layers * lp2 + V2 * H2)
        t_pre, t_dec, t_loop = decode_rate(e, 4, a.prompt, a.new, V2)
        print(f"qwen2.5-7B ({a.qwen25_layers} layers) B=  4: decode {t_dec:6.3f} ms/step = {wb2 / t_dec / 1e6 / 8000:.2f} of HBM peak | device-resident loop "
              f"{t_loop:6.3f} ms/step = {wb2 / t_loop / 1e6 / 8000:.2f} of peak", flush=True)
        e.close()
    sys.exit(0)
H, NH, NKV, INTER, V = 3584, 28, 4, 18944, 152064
t0 = time.time()
from facet_amd.weights import qwen2_5_vl_vision_spec
spec = qwen2_5_vl_text_spec(hidden=H, layers=a.layers, heads=NH, kv_heads=NKV, inter=INTER, vocab=V)
if a.vision or a.from_rgb:
    spec = spec + qwen2_5_vl_vision_spec()      # 32 blocks of 1280 (16 heads of 80), intermediate 3420, merger to 3584
sd = synthetic_state_dict(None, 3, spec=spec)
print(f"weights drawn in {time.time() - t0:.0f} s", flush=True)
e = Engine(0, arena_bytes=40 << 30)
e.vlm_configure(NH, NKV, 128, 1e6, 1e-6, (16, 24, 24))
t0 = time.time()
e.load_weights(FE_MODEL_VLM, sd)
del sd
print(f"committed in {time.time() - t0:.0f} s", flush=True)
if a.scores:
    import ctypes as C
    i32p = C.POINTER(C.c_int32)
    print(f"fe_vlm_generate_scored vs fe_vlm_generate: {a.layers} layers of the 7B geometry + lm_head (vocab {V}), prompt {a.prompt}, "
          f"{a.new} decode steps per call, median of {a.reps} alternating calls each", flush=True)
    for B in [int(b) for b in a.batches.split(",")]:
        L = a.prompt
        p = np.random.default_rng(B).integers(0, V, (B, L)).astype(np.int32)
        tok = np.empty(B, np.int32)
        pos = np.full((3, B), L, np.int32)
        ids = {False: np.empty((a.new, B), np.int32), True: np.empty((a.new, B), np.int32)}
        lp = np.empty((a.new, B), np.float32)
        times = {False: [], True: []}
        for r in range(a.reps + 1):                      # (the first round warms up: graph capture, first-use attributes)
            for scored in (False, True):
                tok[:] = e.vlm_prefill(p, max_seq=L + a.new + 8)
                e.sync()
                t0 = time.perf_counter()
                if scored:
                    e._ck(e.lib.fe_vlm_generate_scored(e.h, tok.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), B, a.new, ids[True].ctypes.data_as(i32p),
                                                       lp.ctypes.data_as(C.POINTER(C.c_float))))
                else:
                    e._ck(e.lib.fe_vlm_generate(e.h, tok.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), B, a.new, ids[False].ctypes.data_as(i32p)))
                dt = (time.perf_counter() - t0) * 1e3 / a.new
                if r:
                    times[scored].append(dt)
            assert np.array_equal(ids[False], ids[True]), "scored and plain loops chose different ids"
        t_p, t_s = float(np.median(times[False])), float(np.median(times[True]))
        print(f"B={B:3d}: plain {t_p:7.4f} ms/step | scored {t_s:7.4f} ms/step | +{(t_s - t_p) * 1e3:6.1f} us/step = {100 * (t_s - t_p) / t_p:+.2f} % "
              f"(spread plain {min(times[False]):.4f}..{max(times[False]):.4f}, scored {min(times[True]):.4f}..{max(times[True]):.4f}); "
              f"ids identical; log-probs {lp.min():.3f}..{lp.max():.3f}", flush=True)
    e.close()
    sys.exit(0)
if a.vision:
    from facet_amd.vlm_tagger import vision_indices
    g = [[1, 74, 74]] * a.vision
    idx = vision_indices(g)
    n = 74 * 74 * a.vision
    pv = np.random.default_rng(0).normal(0, 1, (n, 1176)).astype(np.float32)
    e.vlm_encode_images(pv, idx["patch_pos_hw"], idx["window_index"], idx["cu_window_seqlens"], idx["cu_seqlens"], want_embeds=False)
    e.flops_reset(); e.timer_start()
    e.vlm_encode_images(pv, idx["patch_pos_hw"], idx["window_index"], idx["cu_window_seqlens"], idx["cu_seqlens"], want_embeds=False)
    ms = e.timer_stop()
    print(f"vision tower: {a.vision} images of 74x74 patches ({n // 4 // a.vision} image tokens each) in {ms:.2f} ms = {a.vision / ms * 1e3:.1f} images/s, "
          f"{e.flops() / ms / 1e9:.1f} TFLOP/s (projections; host patches uploaded inside the call)", flush=True)
if a.from_rgb:
    from facet_amd.vlm_tagger import vision_indices, IMAGE_MEAN, IMAGE_STD
    rgb = [np.random.default_rng(i).integers(0, 256, (1036, 1036, 3), dtype=np.uint8) for i in range(a.from_rgb)]
    sizes = [(1036, 1036)] * a.from_rgb
    idx = vision_indices([[1, 74, 74]] * a.from_rgb)
    args = (idx["patch_pos_hw"], idx["window_index"], idx["cu_window_seqlens"], idx["cu_seqlens"])
    pv = e.vlm_preprocess_rgb(rgb, sizes, IMAGE_MEAN, IMAGE_STD, want_pixel_values=True)
    e.vlm_encode_images(pv, *args, want_embeds=False)
    t0 = time.perf_counter(); e.vlm_encode_images(pv, *args, want_embeds=False); t_f32 = (time.perf_counter() - t0) * 1e3
    e.vlm_preprocess_rgb(rgb, sizes, IMAGE_MEAN, IMAGE_STD); e.vlm_encode_preprocessed(*args, want_embeds=False)
    t0 = time.perf_counter()
    e.vlm_preprocess_rgb(rgb, sizes, IMAGE_MEAN, IMAGE_STD)
    t_pre = (time.perf_counter() - t0) * 1e3
    e.vlm_encode_preprocessed(*args, want_embeds=False)
    t_u8 = (time.perf_counter() - t0) * 1e3
    print(f"vision from uint8: {a.from_rgb} photos 1036x1036 -> preprocess {t_pre:.2f} ms (uploads {sum(x.nbytes for x in rgb) / 1e6:.1f} MB) + encode = {t_u8:.2f} ms "
          f"= {a.from_rgb / t_u8 * 1e3:.1f} images/s | fp32 pixel_values upload ({pv.nbytes / 1e6:.0f} MB) + encode {t_f32:.2f} ms = {a.from_rgb / t_f32 * 1e3:.1f} images/s "
          f"(wall clock of the calls)", flush=True)
layer_params = H * (NH + 2 * NKV) * 128 + NH * 128 * H + 3 * H * INTER
head_params = V * H
for B in [int(b) for b in a.batches.split(",")]:
    L = a.prompt
    p = np.random.default_rng(B).integers(0, V, (B, L)).astype(np.int32)
    e.vlm_prefill(p, max_seq=L + a.new + 8)
    e.timer_start(); nxt = e.vlm_prefill(p, max_seq=L + a.new + 8); t_pre = e.timer_stop()
    pos = np.full((3, B), L, np.int32)
    e.vlm_decode_step(nxt, pos)
    t0 = time.perf_counter()
    for s in range(a.new):
        nxt = e.vlm_decode_step(nxt, pos + 1 + s)
    t_dec = (time.perf_counter() - t0) / a.new * 1e3
    # the product path: all decode steps on the device (fe_vlm_generate): one captured graph replayed for <= 2 sequences, stream launches above
    e.vlm_prefill(p, max_seq=L + a.new + 8)
    t0 = time.perf_counter(); e.vlm_generate(p, a.new + 1); t_all = (time.perf_counter() - t0) * 1e3
    t_graph = (t_all - t_pre) / a.new
    fl_pre = 2.0 * (a.layers * layer_params) * B * L + 2.0 * head_params * B + 4.0 * B * NH * L * (L + 1) / 2 * 128 * a.layers
    wbytes = 2.0 * (a.layers * layer_params + head_params)
    full_pre = t_pre * 28 / a.layers
    full_dec = (t_dec - 0) * (28 * layer_params + head_params) / (a.layers * layer_params + head_params)
    print(f"B={B:3d} L={L}: prefill {t_pre:8.2f} ms = {B * L / t_pre * 1e3:9.0f} tok/s, {fl_pre / t_pre / 1e9:7.1f} TFLOP/s ({a.layers} layers; x28/{a.layers}: {full_pre:.1f} ms) | "
          f"decode {t_dec:6.3f} ms/step = {B / t_dec * 1e3:7.0f} tok/s, weights {wbytes / t_dec / 1e6:6.0f} GB/s = {wbytes / t_dec / 1e6 / 8000:.2f} of HBM peak "
          f"(28 layers: ~{full_dec:.2f} ms/step) | device-resident loop (fe_vlm_generate) {t_graph:6.3f} ms/step = {wbytes / t_graph / 1e6:6.0f} GB/s = {wbytes / t_graph / 1e6 / 8000:.2f} of peak", flush=True)
    if a.pad:
        am = np.ones((B, L), np.int32)
        am[1::2, :min(a.pad, L - 1)] = 0
        pp = np.where(am == 1, np.cumsum(am, 1) - 1, 0).astype(np.int32)
        pos3 = np.broadcast_to(pp, (3, B, L))
        e.vlm_prefill(p, pos3, max_seq=L + a.new + 8, pad=(am == 0).sum(1))
        nxt = e.vlm_prefill(p, pos3, max_seq=L + a.new + 8, pad=(am == 0).sum(1))
        posd = np.broadcast_to(pp.max(1) + 1, (3, B)).astype(np.int32)
        e.vlm_decode_step(nxt, posd)
        t0 = time.perf_counter()
        for s in range(a.new):
            nxt = e.vlm_decode_step(nxt, posd + 1 + s)
        t_pd = (time.perf_counter() - t0) / a.new * 1e3
        t0 = time.perf_counter(); e.vlm_generate(p, a.new + 1, position_ids=pos3, attention_mask=am); t_pall = (time.perf_counter() - t0) * 1e3
        print(f"B={B:3d} L={L} padded (every other row {a.pad} pad tokens): decode {t_pd:6.3f} ms/step (unpadded {t_dec:6.3f}) | "
              f"prefill + fe_vlm_generate {t_pall:.2f} ms (unpadded {t_all:.2f})", flush=True)
e.close()
