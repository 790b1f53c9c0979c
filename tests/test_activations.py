"""Sigmoid / Silu / Swish / HardSigmoid / HardSwish / Clip / LeakyRelu / Elu: the C ABI entry points, and the load-time
canonicalisation of a PyTorch-exported MobileNet / EfficientNet-style network.  No device needed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_activation_entry_points_are_exported_and_bound():
    from rten_amd import lib
    so = lib.load()
    for s in ("rten_hip_activation_f32", "rten_hip_gemm_f32_act", "rten_hip_conv2d_f32_act"):
        assert hasattr(so, s), s
        assert s in lib.PROTOTYPES, s
    kinds = [lib.ACT_NONE, lib.ACT_RELU, lib.ACT_GELU, lib.ACT_SIGMOID, lib.ACT_SILU, lib.ACT_SWISH, lib.ACT_HARD_SIGMOID, lib.ACT_HARD_SWISH,
             lib.ACT_CLIP, lib.ACT_LEAKY_RELU, lib.ACT_ELU]
    assert kinds == list(range(11))
    header = open(os.path.join(ROOT, "include", "rten_hip.h")).read()
    for name, v in (("SIGMOID", 3), ("SILU", 4), ("SWISH", 5), ("HARD_SIGMOID", 6), ("HARD_SWISH", 7), ("CLIP", 8), ("LEAKY_RELU", 9), ("ELU", 10)):
        assert f"#define RTEN_HIP_ACT_{name} {v} " in header, name


def test_python_operators_carry_the_reference_defaults():
    from rten_amd import lib, ops
    assert (ops.Swish().kind, ops.Swish().alpha) == (lib.ACT_SWISH, 1.0)
    assert (ops.HardSigmoid().alpha, ops.HardSigmoid().beta) == (0.2, 0.5)
    assert ops.LeakyRelu().alpha == 0.01 and ops.Elu().alpha == 1.0
    c = ops.Clip()
    assert c.alpha == -c.beta and c.beta == float(__import__("numpy").finfo("float32").max)
    assert ops._activation_args(ops.Clip(0, 6)) == (lib.ACT_CLIP, 0.0, 6.0)


def _canonical_line(tmp_path, model_bytes):
    from tests.test_graph_executor import run_cli
    p = tmp_path / "m.onnx"
    p.write_bytes(model_bytes)
    out = run_cli("--parse-only", str(p))
    assert out.returncode == 0, out.stderr
    raw = [l for l in out.stdout.splitlines() if "operators:" in l][0]
    canon = [l for l in out.stdout.splitlines() if "canonical form" in l][0]
    return raw, canon


def test_pytorch_exported_mobile_network_canonical_form(tmp_path):
    """ReLU6 -> Clip (min / max attributes), SiLU -> Sigmoid + Mul, QuickGELU x * sigmoid(1.702 x), Hardsigmoid / Sigmoid
    squeeze-excite gates: the SiluFusion / SwishFusion patterns leave Silu x3 and Swish x1, and the only Sigmoid left is the
    squeeze-excite gate."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export as te
    raw, canon = _canonical_line(tmp_path, te.mobile_onnx())
    assert "Clip x2" in raw and "Sigmoid x5" in raw and "LeakyRelu x1" in raw and "Elu x1" in raw and "GlobalAveragePool x3" in raw
    body = canon.split("nodes:")[1]
    assert "Silu x3" in body and "Swish x1" in body and "Sigmoid x1" in body, canon
    assert "Clip x2" in body and "Mul x3" in body  # two squeeze-excite gates and Hardswish's x * HardSigmoid(x)


def test_silu_swish_patterns_in_either_operand_order(tmp_path):
    import numpy as np
    from rten_amd import onnx_writer as ow
    nodes = [ow.node("Sigmoid", ["x"], ["s"], name="sig"),
             ow.node("Mul", ["s", "x"], ["a"], name="silu_rev"),        # Sigmoid(x) * x
             ow.node("Mul", ["alpha", "a"], ["ax"], name="scale"),      # alpha * a
             ow.node("Sigmoid", ["ax"], ["s2"], name="sig2"),
             ow.node("Mul", ["a", "s2"], ["b"], name="swish"),          # a * Sigmoid(alpha * a)
             ow.node("Sigmoid", ["b"], ["s3"], name="gate"),             # Sigmoid(b) * c: not a Silu
             ow.node("Mul", ["s3", "c"], ["y"], name="gated")]
    m = ow.model(nodes, [ow.value_info("x", ow.FLOAT, [2, 8]), ow.value_info("c", ow.FLOAT, [2, 8])], [ow.value_info("y", ow.FLOAT, [2, 8])],
                 [ow.tensor("alpha", np.array(1.702, np.float32))])
    _, canon = _canonical_line(tmp_path, m)
    body = canon.split("nodes:")[1]
    assert "Silu x1" in body and "Swish x1" in body and "Sigmoid x1" in body and "Mul x1" in body, canon
