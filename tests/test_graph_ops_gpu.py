"""GPU: the ONNX graph runtime (facet_amd/csrc/onnx_graph.hip, kernels_graph.hip and the shared kernels it calls) operator by operator, attribute by
attribute and layout by layout against the float64 references of tests/graph_ops_ref.py. The graphs are those of tests/graph_ops_cases.py
(tests/test_graph_ops_host.py holds them to torch and to themselves): one operator each, or the shortest chain that reaches it, every value of
interest declared as a graph output and every output judged against the reference of ITS operator on the inputs the runtime itself returned.

Check: the output's shape; bit equality where the operator only moves or selects values (Relu, MaxPool, nearest Resize, Concat, Flatten,
Transpose, Reshape, Squeeze, Unsqueeze, Identity, Dropout); otherwise |got - ref| <= A + ulp32(ref) / 2 elementwise with the bounds A derived in
graph_ops_ref.py's docstring, and a finite result. All graphs go through one context and one slot: loaded, run at a batch of 2, then of 3
(the per-node caches are keyed on the channel count and must serve both), unloaded. Each test prints its worst err / bound per operator before
it asserts (DESIGN.md records them)."""
import numpy as np
import pytest

import graph_ops_cases as C
import graph_ops_ref as G
import plain_ops_ref as R

pytestmark = pytest.mark.gpu

SLOT = 3


def _run_case(engine, w, case):
    engine.graph_load(SLOT, case.data)
    try:
        for n in (2, 3):
            x = case.input(n)
            outs = engine.graph_run(SLOT, x.astype(np.float32))
            assert len(outs) == len(case.checks), (case.name, len(outs))
            for chk, got, ref, A in C.evaluate(case, x, outs):
                what = f"{case.name} {chk.name} n={n}"
                if got.shape != ref.shape:
                    w.fails.append(f"{chk.key} {what}: shape {got.shape} != {ref.shape}")
                elif A is None:
                    w.exact(chk.key, what, got.astype(np.float64), ref)
                else:
                    w.close(chk.key, what, got, ref, A + G.ulp32(ref) / 2)
    finally:
        engine.graph_unload(SLOT)


@pytest.mark.parametrize("family", C.FAMILIES)
def test_family(engine, family):
    """activations: standalone on maps of 3 / 6 / 20 / 21 channels and on reshaped tensors whose element count is no multiple of 4, LeakyRelu with
    and without alpha, PRelu slopes as [C], [C,1,1], [1,C,1,1] and scalar, BatchNormalization alone and with each activation behind it.
    binary: the four operators map (op) map at 6 and 21 channels, map (op) scalar / [C,1,1] / [1,C,1,1], the constant on the left, reshaped tensors.
    fusion: every shape of group the planner builds (graph_ops_cases._fusion). depthwise: 3x3 and 5x5, strides, pads, bias, BatchNormalization; and
    the dense convolutions with strides, pads and dilations. pools: k, s, p, ceil_mode, count_include_pad; GlobalAveragePool. resize: nearest and
    linear, sizes and whole-pixel scales, both coordinate modes, the opset-10 and Upsample forms. layout: Concat, Transpose, Reshape, Squeeze,
    Unsqueeze, Flatten -> Gemm, MatMul. softmax: ranks 2 - 4, opsets 11 and 13, rows of 1, 7, 200. hygiene: maps with 0.5, NaN or Inf candidates
    in their padding lanes into every class of consumer."""
    w = R.Worst(f"graph ops: {family}")
    cases = [c for c in C.CASES if c.family == family]
    assert cases
    for case in cases:
        _run_case(engine, w, case)
    w.report()


def test_rejected_graphs_raise_and_leave_the_context_usable(engine):
    """Sub and Div with the constant on the left, dilated depthwise Conv, Resize by scales that do not give whole pixels (1.3 and 1.5 on h = 5),
    pytorch_half_pixel with an output length of 1, nearest with round_prefer_floor (given, and as the opset-11 default) or half_pixel,
    align_corners and cubic: EngineError with a message that names the node's problem; after each, a graph runs in the same slot."""
    from facet_amd._lib import EngineError
    probe = next(c for c in C.CASES if c.name == "resize_opset10")
    w = R.Worst("graph ops: after a rejected graph")
    for r in C.REJECTED:
        engine.graph_load(SLOT, r.data)
        with pytest.raises(EngineError, match=r.match):
            engine.graph_run(SLOT, r.net.input(2).astype(np.float32))
        engine.graph_unload(SLOT)
        _run_case(engine, w, probe)
    w.report()
