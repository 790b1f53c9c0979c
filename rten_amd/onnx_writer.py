"""Minimal ONNX writer (protobuf wire format by hand) -- SURVEY 8(f) rank 3, "model tooling without ORT".

There is no `onnx` / `onnxruntime` package on the GPU boxes, so the named configs are manufactured here: graphs are
serialised directly in the ONNX protobuf encoding (onnx.proto3 field numbers quoted below) and read back by the C++
loader in include/rten_hip_graph.hpp (the backend's counterpart of rten-onnx/src/onnx.rs + src/model/onnx_loader.rs).

Also restated here: the weight side of ort's `quantize_dynamic(..., reduce_range=True)` as RTen's tools/ort-quantize.py
drives it (tools/ort-quantize.py:100-151) -- per-tensor symmetric 7-bit weights, DynamicQuantizeLinear on activations,
ConvInteger / MatMulInteger -> Cast -> Mul(x_scale * w_scale) -> Add(bias).
"""
from __future__ import annotations

import struct

import numpy as np

# TensorProto.DataType
FLOAT, UINT8, INT8, INT32, INT64 = 1, 2, 3, 6, 7
_NP2ONNX = {np.dtype(np.float32): FLOAT, np.dtype(np.uint8): UINT8, np.dtype(np.int8): INT8, np.dtype(np.int32): INT32, np.dtype(np.int64): INT64}


def _varint(n: int) -> bytes:
    n &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field: int, wire: int) -> bytes:
    return _varint((field << 3) | wire)


def _ld(field: int, payload: bytes) -> bytes:  # length-delimited
    return _key(field, 2) + _varint(len(payload)) + payload


def _vi(field: int, v: int) -> bytes:
    return _key(field, 0) + _varint(int(v))


def _str(field: int, s: str) -> bytes:
    return _ld(field, s.encode())


def tensor(name: str, arr) -> bytes:
    """TensorProto: dims = 1, data_type = 2, name = 8, raw_data = 9."""
    a = np.asarray(arr)
    if a.ndim and not a.flags.c_contiguous:  # (ascontiguousarray would turn a 0-d scalar into shape [1])
        a = np.ascontiguousarray(a)
    out = b"".join(_vi(1, d) for d in a.shape)
    out += _vi(2, _NP2ONNX[a.dtype]) + _str(8, name) + _ld(9, a.tobytes())
    return out


def attr(name: str, value) -> bytes:
    """AttributeProto: name = 1, f = 2, i = 3, s = 4, t = 5, floats = 7, ints = 8, type = 20
    (AttributeType FLOAT = 1, INT = 2, STRING = 3, TENSOR = 4, FLOATS = 6, INTS = 7), strings = 9 (STRINGS = 8)."""
    out = _str(1, name)
    if isinstance(value, bool) or isinstance(value, (int, np.integer)):
        return out + _vi(3, int(value)) + _vi(20, 2)
    if isinstance(value, (float, np.floating)):
        return out + _key(2, 5) + struct.pack("<f", float(value)) + _vi(20, 1)
    if isinstance(value, (bytes, str)):
        return out + _ld(4, value.encode() if isinstance(value, str) else value) + _vi(20, 3)
    if isinstance(value, np.ndarray):
        return out + _ld(5, tensor("", value)) + _vi(20, 4)
    value = list(value)
    if value and all(isinstance(v, str) for v in value):
        return out + b"".join(_ld(9, v.encode()) for v in value) + _vi(20, 8)
    if all(isinstance(v, (int, np.integer)) for v in value):
        return out + b"".join(_vi(8, int(v)) for v in value) + _vi(20, 7)
    return out + b"".join(_key(7, 5) + struct.pack("<f", float(v)) for v in value) + _vi(20, 6)


def node(op_type: str, inputs, outputs, name: str = "", domain: str = "", **attrs) -> bytes:
    """NodeProto: input = 1, output = 2, name = 3, op_type = 4, attribute = 5, domain = 7."""
    out = b"".join(_str(1, i) for i in inputs) + b"".join(_str(2, o) for o in outputs)
    if name:
        out += _str(3, name)
    out += _str(4, op_type)
    out += b"".join(_ld(5, attr(k, v)) for k, v in attrs.items())
    if domain:
        out += _str(7, domain)
    return out


def value_info(name: str, elem_type: int, shape) -> bytes:
    """ValueInfoProto: name = 1, type = 2 { tensor_type = 1 { elem_type = 1, shape = 2 { dim = 1 { dim_value = 1 | dim_param = 2 } } } }."""
    dims = b"".join(_ld(1, _str(2, d) if isinstance(d, str) else _vi(1, d)) for d in shape)
    ttype = _vi(1, elem_type) + _ld(2, dims)
    return _str(1, name) + _ld(2, _ld(1, ttype))


def model(nodes, inputs, outputs, initializers, opset: int = 17, name: str = "graph", producer: str = "rten_amd.onnx_writer") -> bytes:
    """ModelProto: ir_version = 1, producer_name = 2, graph = 7, opset_import = 8 { domain = 1, version = 2 };
    GraphProto: node = 1, name = 2, initializer = 5, input = 11, output = 12."""
    g = b"".join(_ld(1, n) for n in nodes) + _str(2, name) + b"".join(_ld(5, t) for t in initializers)
    g += b"".join(_ld(11, v) for v in inputs) + b"".join(_ld(12, v) for v in outputs)
    return _vi(1, 8) + _str(2, producer) + _ld(7, g) + _ld(8, _str(1, "") + _vi(2, opset))


# ----------------------------------------------------------------------------------------------------------------
# ResNet-50 v1.5 (BASELINE configs[0..2]) as an exporter would write it: BN folded, Conv / Relu / Add as separate nodes
# ----------------------------------------------------------------------------------------------------------------

def resnet50_f32(weights, batch="batch", image: int = 224) -> bytes:
    from .workloads.resnet50 import conv_specs
    nodes, inits = [], []
    for l in conv_specs():
        w, b = weights[l["name"]]
        inits += [tensor(l["name"] + ".w", w), tensor(l["name"] + ".b", b)]
        conv_out = l["dst"] + ".conv" if (l["relu"] or l["res"]) else l["dst"]
        nodes.append(node("Conv", [l["src"], l["name"] + ".w", l["name"] + ".b"], [conv_out], name=l["name"], dilations=[1, 1], group=1,
                          kernel_shape=[l["k"], l["k"]], pads=[l["pad"]] * 4, strides=[l["stride"]] * 2))
        cur = conv_out
        if l["res"]:
            nxt = l["dst"] + ".sum" if l["relu"] else l["dst"]
            nodes.append(node("Add", [cur, l["res"]], [nxt], name=l["name"] + ".add"))
            cur = nxt
        if l["relu"]:
            nodes.append(node("Relu", [cur], [l["dst"]], name=l["name"] + ".relu"))
        if l["name"] == "stem":
            nodes.append(node("MaxPool", ["stem"], ["pool"], name="maxpool", ceil_mode=0, kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]))
    last = conv_specs()[-1]["dst"]
    fw, fb = weights["fc"]
    inits += [tensor("fc.w", fw), tensor("fc.b", fb)]
    nodes.append(node("GlobalAveragePool", [last], ["gap"], name="gap"))
    nodes.append(node("Flatten", ["gap"], ["flat"], name="flatten", axis=1))
    nodes.append(node("Gemm", ["flat", "fc.w", "fc.b"], ["logits"], name="fc", alpha=1.0, beta=1.0, transB=1))
    return model(nodes, [value_info("x", FLOAT, [batch, 3, image, image])], [value_info("logits", FLOAT, [batch, fw.shape[0]])], inits, name="resnet50")


def quantize_weight_reduce_range(w):
    """Per-tensor symmetric weight quantisation of ort's dynamic quantiser with reduce_range=True (7-bit, [-64, 64]):
    scale = max|w| / 64, q = clip(rint(w / scale)), zero point 0 (tools/ort-quantize.py:124-137)."""
    s = np.float32(np.abs(w).max() / 64.0)
    return np.clip(np.rint(w / s), -64, 64).astype(np.int8), s


def resnet50_int8(weights, batch="batch", image: int = 224) -> bytes:
    """The same network after dynamic quantisation: per Conv
        DynamicQuantizeLinear(x) -> ConvInteger(xq, wq, x_zp, w_zp) -> Cast(FLOAT) -> Mul(Mul(x_scale, w_scale)) -> Add(bias [1,O,1,1])
    one DynamicQuantizeLinear per distinct input tensor (the quantiser caches quantised inputs), bias as a separate Add
    (SURVEY 8d config 3), the classifier as MatMulInteger."""
    from .workloads.resnet50 import conv_specs
    nodes, inits, quantized = [], [], set()

    def dql(src):
        if src not in quantized:
            nodes.append(node("DynamicQuantizeLinear", [src], [src + ".q", src + ".scale", src + ".zp"], name=src + ".dql"))
            quantized.add(src)
        return src + ".q", src + ".scale", src + ".zp"

    inits.append(tensor("zero_i8", np.zeros((), np.int8)))
    for l in conv_specs():
        w, b = weights[l["name"]]
        wq, ws = quantize_weight_reduce_range(w)
        n = l["name"]
        inits += [tensor(n + ".wq", wq), tensor(n + ".ws", np.array(ws, np.float32)), tensor(n + ".b", b.reshape(1, -1, 1, 1))]
        xq, xs, xz = dql(l["src"])
        nodes.append(node("ConvInteger", [xq, n + ".wq", xz, "zero_i8"], [n + ".acc"], name=n, dilations=[1, 1], group=1, kernel_shape=[l["k"], l["k"]],
                          pads=[l["pad"]] * 4, strides=[l["stride"]] * 2))
        nodes.append(node("Cast", [n + ".acc"], [n + ".accf"], name=n + ".cast", to=FLOAT))
        nodes.append(node("Mul", [xs, n + ".ws"], [n + ".scale"], name=n + ".scale_mul"))
        nodes.append(node("Mul", [n + ".accf", n + ".scale"], [n + ".scaled"], name=n + ".mul"))
        cur = l["dst"] + ".biased" if (l["relu"] or l["res"]) else l["dst"]
        nodes.append(node("Add", [n + ".scaled", n + ".b"], [cur], name=n + ".bias"))
        if l["res"]:
            nxt = l["dst"] + ".sum" if l["relu"] else l["dst"]
            nodes.append(node("Add", [cur, l["res"]], [nxt], name=n + ".add"))
            cur = nxt
        if l["relu"]:
            nodes.append(node("Relu", [cur], [l["dst"]], name=n + ".relu"))
        if n == "stem":
            nodes.append(node("MaxPool", ["stem"], ["pool"], name="maxpool", ceil_mode=0, kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]))
    last = conv_specs()[-1]["dst"]
    fw, fb = weights["fc"]
    fq, fs = quantize_weight_reduce_range(fw)
    inits += [tensor("fc.wq", np.ascontiguousarray(fq.T)), tensor("fc.ws", np.array(fs, np.float32)), tensor("fc.b", fb)]
    nodes.append(node("GlobalAveragePool", [last], ["gap"], name="gap"))
    nodes.append(node("Flatten", ["gap"], ["flat"], name="flatten", axis=1))
    xq, xs, xz = dql("flat")
    nodes.append(node("MatMulInteger", [xq, "fc.wq", xz, "zero_i8"], ["fc.acc"], name="fc"))
    nodes.append(node("Cast", ["fc.acc"], ["fc.accf"], name="fc.cast", to=FLOAT))
    nodes.append(node("Mul", [xs, "fc.ws"], ["fc.scale"], name="fc.scale_mul"))
    nodes.append(node("Mul", ["fc.accf", "fc.scale"], ["fc.scaled"], name="fc.mul"))
    nodes.append(node("Add", ["fc.scaled", "fc.b"], ["logits"], name="fc.bias"))
    return model(nodes, [value_info("x", FLOAT, [batch, 3, image, image])], [value_info("logits", FLOAT, [batch, fw.shape[0]])], inits, name="resnet50_int8")


def small_cnn_f32(seed: int = 7):
    """A few-layer CNN with every node kind of the ResNet graph (tests): returns (model bytes, weights dict)."""
    rng = np.random.default_rng(seed)
    w = {"c1": (rng.normal(0, 0.3, (8, 3, 3, 3)).astype(np.float32), rng.normal(0, 0.1, 8).astype(np.float32)),
         "c2": (rng.normal(0, 0.2, (8, 8, 1, 1)).astype(np.float32), rng.normal(0, 0.1, 8).astype(np.float32)),
         "fc": (rng.normal(0, 0.3, (5, 8)).astype(np.float32), rng.normal(0, 0.1, 5).astype(np.float32))}
    inits = [tensor("c1.w", w["c1"][0]), tensor("c1.b", w["c1"][1]), tensor("c2.w", w["c2"][0]), tensor("c2.b", w["c2"][1]),
             tensor("fc.w", w["fc"][0]), tensor("fc.b", w["fc"][1])]
    nodes = [node("Conv", ["x", "c1.w", "c1.b"], ["a"], name="c1", kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]),
             node("Relu", ["a"], ["a.r"], name="c1.relu"),
             node("MaxPool", ["a.r"], ["p"], name="pool", kernel_shape=[2, 2], strides=[2, 2]),
             node("Conv", ["p", "c2.w", "c2.b"], ["b"], name="c2", kernel_shape=[1, 1]),
             node("Add", ["b", "p"], ["s"], name="add"),
             node("Relu", ["s"], ["s.r"], name="relu"),
             node("GlobalAveragePool", ["s.r"], ["g"], name="gap"),
             node("Flatten", ["g"], ["f"], name="flatten", axis=1),
             node("Gemm", ["f", "fc.w", "fc.b"], ["y"], name="fc", transB=1)]
    return model(nodes, [value_info("x", FLOAT, ["batch", 3, 16, 16])], [value_info("y", FLOAT, ["batch", 5])], inits, name="small_cnn"), w


# ----------------------------------------------------------------------------------------------------------------
# BERT encoder (BASELINE configs[3]) in the shape an exporter gives it: separate Q / K / V projections, Reshape /
# Transpose around the attention MatMuls, Div by sqrt(d), Add(mask) -> Softmax, LayerNormalization (opset 17), Gelu
# ----------------------------------------------------------------------------------------------------------------

def bert_encoder(cfg, weights, seq: int, batch="batch") -> bytes:
    """inputs: input_ids, token_type_ids, attention_mask -- int64 [batch, seq]; output: last_hidden_state [batch, seq, hidden]."""
    return _bert_encoder(cfg, weights, seq, batch, [], [], None)


def _bert_encoder(cfg, weights, seq, batch, nodes, inits, weight_matmul) -> bytes:
    """`weight_matmul(nodes, inits, x, weight name, out, node name)`: writes the MatMul of an activation with a weight (bert_encoder_qdq puts its
    Q/DQ nodes there); None = a plain MatMul over the f32 initializer."""
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh
    w = weights

    def wmm(x, wname, out, name):
        if weight_matmul is None:
            nodes.append(node("MatMul", [x, wname], [out], name=name))
        else:
            weight_matmul(nodes, inits, x, wname, out, name)

    def const(name, arr):
        inits.append(tensor(name, arr))
        return name

    const("word", w["word"]); const("type", w["type"]); const("pos", np.ascontiguousarray(w["pos"][:seq]))
    const("emb_ln_g", w["emb_ln_g"]); const("emb_ln_b", w["emb_ln_b"])
    const("one", np.array(1.0, np.float32)); const("f32_min", np.array(np.finfo(np.float32).min, np.float32))
    const("sqrt_dh", np.array(np.sqrt(np.float32(dh)), np.float32))
    const("mask_axes", np.array([1, 2], np.int64))
    const("split_heads", np.array([0, 0, nh, dh], np.int64)); const("merge_heads", np.array([0, 0, H], np.int64))
    # embeddings
    nodes.append(node("Gather", ["word", "input_ids"], ["emb.word"], name="emb.word", axis=0))
    nodes.append(node("Gather", ["type", "token_type_ids"], ["emb.type"], name="emb.type", axis=0))
    nodes.append(node("Add", ["emb.word", "emb.type"], ["emb.wt"], name="emb.add_type"))
    nodes.append(node("Add", ["emb.wt", "pos"], ["emb.sum"], name="emb.add_pos"))
    nodes.append(node("LayerNormalization", ["emb.sum", "emb_ln_g", "emb_ln_b"], ["x0"], name="emb.ln", axis=-1, epsilon=float(cfg.eps)))
    # additive attention mask: (1 - mask) * finfo(f32).min as [B, 1, 1, S]
    nodes.append(node("Unsqueeze", ["attention_mask", "mask_axes"], ["mask.4d"], name="mask.unsqueeze"))
    nodes.append(node("Cast", ["mask.4d"], ["mask.f"], name="mask.cast", to=FLOAT))
    nodes.append(node("Sub", ["one", "mask.f"], ["mask.inv"], name="mask.sub"))
    nodes.append(node("Mul", ["mask.inv", "f32_min"], ["mask.bias"], name="mask.mul"))
    x = "x0"
    for i, lw in enumerate(w["layers"]):
        p = f"l{i}."
        for k in ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2", "ln2_g", "ln2_b"):
            if weight_matmul is None or k not in ("wq", "wk", "wv", "wo", "w1", "w2"):
                const(p + k, lw[k])
        for t in ("q", "k", "v"):
            wmm(x, p + "w" + t, p + t + ".mm", p + t + ".matmul")
            nodes.append(node("Add", [p + t + ".mm", p + "b" + t], [p + t + ".lin"], name=p + t + ".bias"))
            nodes.append(node("Reshape", [p + t + ".lin", "split_heads"], [p + t + ".4d"], name=p + t + ".reshape"))
            nodes.append(node("Transpose", [p + t + ".4d"], [p + t], name=p + t + ".transpose", perm=[0, 2, 3, 1] if t == "k" else [0, 2, 1, 3]))
        nodes.append(node("MatMul", [p + "q", p + "k"], [p + "scores.raw"], name=p + "qk"))
        nodes.append(node("Div", [p + "scores.raw", "sqrt_dh"], [p + "scores"], name=p + "scale"))
        nodes.append(node("Add", [p + "scores", "mask.bias"], [p + "scores.masked"], name=p + "mask"))
        nodes.append(node("Softmax", [p + "scores.masked"], [p + "probs"], name=p + "softmax", axis=-1))
        nodes.append(node("MatMul", [p + "probs", p + "v"], [p + "ctx.h"], name=p + "pv"))
        nodes.append(node("Transpose", [p + "ctx.h"], [p + "ctx.t"], name=p + "ctx.transpose", perm=[0, 2, 1, 3]))
        nodes.append(node("Reshape", [p + "ctx.t", "merge_heads"], [p + "ctx"], name=p + "ctx.reshape"))
        wmm(p + "ctx", p + "wo", p + "o.mm", p + "o.matmul")
        nodes.append(node("Add", [p + "o.mm", p + "bo"], [p + "o.lin"], name=p + "o.bias"))
        nodes.append(node("Add", [p + "o.lin", x], [p + "res1"], name=p + "res1"))
        nodes.append(node("LayerNormalization", [p + "res1", p + "ln1_g", p + "ln1_b"], [p + "x1"], name=p + "ln1", axis=-1, epsilon=float(cfg.eps)))
        wmm(p + "x1", p + "w1", p + "h.mm", p + "ffn1.matmul")
        nodes.append(node("Add", [p + "h.mm", p + "b1"], [p + "h.lin"], name=p + "ffn1.bias"))
        nodes.append(node("Gelu", [p + "h.lin"], [p + "h"], name=p + "gelu"))
        wmm(p + "h", p + "w2", p + "f.mm", p + "ffn2.matmul")
        nodes.append(node("Add", [p + "f.mm", p + "b2"], [p + "f.lin"], name=p + "ffn2.bias"))
        nodes.append(node("Add", [p + "f.lin", p + "x1"], [p + "res2"], name=p + "res2"))
        out = "last_hidden_state" if i == len(w["layers"]) - 1 else p + "x2"
        nodes.append(node("LayerNormalization", [p + "res2", p + "ln2_g", p + "ln2_b"], [out], name=p + "ln2", axis=-1, epsilon=float(cfg.eps)))
        x = out
    ins = [value_info(n, INT64, [batch, seq]) for n in ("input_ids", "token_type_ids", "attention_mask")]
    return model(nodes, ins, [value_info("last_hidden_state", FLOAT, [batch, seq, H])], inits, opset=20, name="bert_encoder")


# ----------------------------------------------------------------------------------------------------------------
# Static quantisation in ONNX Runtime's QDQ layout (`quantize_static`, QuantFormat.QDQ): int8 weights and int32 biases behind a
# DequantizeLinear each, a QuantizeLinear -> DequantizeLinear pair on the activations.  The scales come from a min/max calibration
# pass over the f32 network, run here in numpy on seeded inputs.
# ----------------------------------------------------------------------------------------------------------------

def activation_qparams(lo, hi):
    """ort's asymmetric u8 parameters of a calibrated range (the range is widened to contain 0): scale, zero point."""
    lo, hi = min(float(lo), 0.0), max(float(hi), 0.0)
    scale = np.float32((hi - lo) / 255.0) if hi > lo else np.float32(1.0)
    zp = np.uint8(np.clip(np.rint(-lo / float(scale)), 0, 255))
    return scale, zp


def quantize_weight_per_channel(w, axis):
    """Symmetric int8 weights, one scale per slice of `axis`: scale = max|w| / 127, q = clip(rint(w / scale), -127, 127), zero points 0."""
    red = tuple(d for d in range(w.ndim) if d != axis)
    s = (np.abs(w).max(axis=red) / 127.0).astype(np.float32)
    s = np.where(s == 0, np.float32(1.0), s).astype(np.float32)
    shape = [1] * w.ndim
    shape[axis] = -1
    q = np.clip(np.rint(w / s.reshape(shape)), -127, 127).astype(np.int8)
    return q, s, np.zeros(s.shape, np.int8)


def quantize_weight_per_tensor(w):
    s = np.float32(np.abs(w).max() / 127.0) or np.float32(1.0)
    return np.clip(np.rint(w / s), -127, 127).astype(np.int8), np.float32(s), np.int8(0)


class _QdqGraph:
    """Node / initializer lists plus the Q/DQ bookkeeping of a QDQ builder.  `q` records every quantised constant and every activation's parameters
    by name, so that a test can restate the graph with its own operators."""

    def __init__(self, enabled=True):
        self.nodes, self.inits, self.q = [], [], {"act": {}, "weight": {}, "bias": {}}
        self._pairs = {}
        self.enabled = enabled  # False: the same network in f32 (no Q/DQ node, f32 initializers): the twin a QDQ graph's time is read against

    def const(self, name, arr):
        self.inits.append(tensor(name, arr))
        return name

    def pair(self, src, lo_hi, dequantize=True):
        """QuantizeLinear -> DequantizeLinear on `src` with per-tensor u8 constants (one pair per tensor, shared by its readers)."""
        if not self.enabled:
            return src
        if src not in self._pairs:
            scale, zp = activation_qparams(*lo_hi)
            self.q["act"][src] = (scale, zp)
            self.const(src + ".scale", np.array(scale, np.float32))
            self.const(src + ".zp", np.array(zp, np.uint8))
            self.nodes.append(node("QuantizeLinear", [src, src + ".scale", src + ".zp"], [src + ".q"], name=src + ".quant"))
            if dequantize:
                self.nodes.append(node("DequantizeLinear", [src + ".q", src + ".scale", src + ".zp"], [src + ".dq"], name=src + ".dequant"))
            self._pairs[src] = src + ".dq" if dequantize else src + ".q"
        return self._pairs[src]

    def weight(self, name, w, axis=None):
        """int8 weight behind a DequantizeLinear: per slice of `axis`, or per-tensor (axis None)."""
        if not self.enabled:
            return self.const(name, w), None
        wq, ws, wz = quantize_weight_per_tensor(w) if axis is None else quantize_weight_per_channel(w, axis)
        self.q["weight"][name] = (wq, ws, wz, axis)
        self.const(name + ".q", wq); self.const(name + ".scale", np.asarray(ws, np.float32)); self.const(name + ".zp", np.asarray(wz, np.int8))
        self.nodes.append(node("DequantizeLinear", [name + ".q", name + ".scale", name + ".zp"], [name + ".dq"], name=name + ".dequant", **({} if axis is None else {"axis": axis})))
        return name + ".dq", ws

    def bias(self, name, b, x_scale, w_scale):
        """int32 bias with scale x_scale * w_scale[c] and no zero point."""
        if not self.enabled:
            return self.const(name, b)
        bs = (np.float32(x_scale) * np.asarray(w_scale, np.float32).reshape(-1)).astype(np.float32)
        if bs.size == 1:
            bs = np.repeat(bs, b.size)
        bq = np.clip(np.rint(b.astype(np.float64) / bs), -(2 ** 31), 2 ** 31 - 1).astype(np.int32)
        self.q["bias"][name] = (bq, bs)
        self.const(name + ".q", bq); self.const(name + ".scale", bs)
        self.nodes.append(node("DequantizeLinear", [name + ".q", name + ".scale"], [name + ".dq"], name=name + ".dequant", axis=0))
        return name + ".dq"


def _np_conv2d(x, w, b, stride=1, pad=0, groups=1):
    """Plain numpy convolution (calibration only: its rounding is not the device's)."""
    n, c, h, wd = x.shape
    o, cg, kh, kw = w.shape
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    win = np.lib.stride_tricks.sliding_window_view(xp, (kh, kw), axis=(2, 3))[:, :, ::stride, ::stride]  # [n, c, oh, ow, kh, kw]
    og = o // groups
    out = [np.einsum("nchwij,ocij->nohw", win[:, g * cg:(g + 1) * cg], w[g * og:(g + 1) * og]) for g in range(groups)]
    return (np.concatenate(out, 1) + b.reshape(1, -1, 1, 1)).astype(np.float32)


def small_cnn_qdq_weights(seed: int = 9):
    rng = np.random.default_rng(seed)
    n = lambda std, *s: rng.normal(0, std, s).astype(np.float32)
    return {"stem": (n(0.3, 8, 3, 3, 3), n(0.1, 8)), "b1": (n(0.15, 8, 8, 3, 3), n(0.1, 8)), "b2": (n(0.15, 8, 8, 3, 3), n(0.1, 8)),
            "dw": (n(0.3, 8, 1, 3, 3), n(0.1, 8)), "fc": (n(0.3, 5, 8), n(0.1, 5))}


def small_cnn_qdq(seed: int = 9, image: int = 16, quantized_output: bool = False, quantize: bool = True):
    """A small CNN after static quantisation in the QDQ layout: stem conv, one residual block (Conv+Relu, Conv, Add, Relu), a depthwise conv, MaxPool,
    GlobalAveragePool and a Gemm with transB.  u8 activations with per-tensor constants, i8 weights per output channel (axis 0), int32 biases with scale
    x_scale * w_scale[c] and no zero point.  A Q/DQ pair sits on the graph input, behind every convolution group (the pair follows the group's Relu, and
    the residual Add and its Relu stay next to their convolution, as ort places the pair behind a fused activation), behind both pools and on the logits.
    `quantized_output`: the graph output is the quantised logits (u8), without the last DequantizeLinear.  `quantize=False`: the f32 network itself
    (output "logits"), the twin a QDQ graph's time is read against.
    -> (model bytes, q): q["act"][tensor] = (scale, zero point), q["weight"][name] = (wq, scale, zero point, axis), q["bias"][name] = (bq, scale),
    q["folded"] = the number of DequantizeLinear nodes over initializers."""
    w = small_cnn_qdq_weights(seed)
    # calibration: the f32 network on seeded inputs
    x = np.random.default_rng(seed + 1).normal(0, 1, (4, 3, image, image)).astype(np.float32)
    relu = lambda t: np.maximum(t, 0)
    a = relu(_np_conv2d(x, *w["stem"], stride=2, pad=1))
    b = relu(_np_conv2d(a, *w["b1"], pad=1))
    s = relu(_np_conv2d(b, *w["b2"], pad=1) + a)
    d = _np_conv2d(s, *w["dw"], pad=1, groups=8)
    p = d.reshape(d.shape[0], 8, d.shape[2] // 2, 2, d.shape[3] // 2, 2).max(axis=(3, 5))
    gp = p.mean(axis=(2, 3), keepdims=True)
    y = gp.reshape(gp.shape[0], -1) @ w["fc"][0].T + w["fc"][1]
    rng_of = lambda t: (t.min(), t.max())

    g = _QdqGraph(quantize)

    def conv(name, src, src_range, dst, **attrs):
        xin = g.pair(src, src_range)
        wd, ws = g.weight(name + ".w", w[name][0], axis=0)
        bd = g.bias(name + ".b", w[name][1], g.q["act"].get(src, (None,))[0], ws)
        g.nodes.append(node("Conv", [xin, wd, bd], [dst], name=name, kernel_shape=[3, 3], **attrs))

    conv("stem", "x", rng_of(x), "a.conv", pads=[1, 1, 1, 1], strides=[2, 2])
    g.nodes.append(node("Relu", ["a.conv"], ["a"], name="stem.relu"))
    conv("b1", "a", rng_of(a), "b.conv", pads=[1, 1, 1, 1])
    g.nodes.append(node("Relu", ["b.conv"], ["b"], name="b1.relu"))
    conv("b2", "b", rng_of(b), "s.conv", pads=[1, 1, 1, 1])
    g.nodes.append(node("Add", ["s.conv", g.pair("a", rng_of(a))], ["s.sum"], name="b2.add"))
    g.nodes.append(node("Relu", ["s.sum"], ["s"], name="b2.relu"))
    conv("dw", "s", rng_of(s), "d", pads=[1, 1, 1, 1], group=8)
    g.nodes.append(node("MaxPool", [g.pair("d", rng_of(d))], ["p"], name="pool", kernel_shape=[2, 2], strides=[2, 2]))
    g.nodes.append(node("GlobalAveragePool", [g.pair("p", rng_of(p))], ["g"], name="gap"))
    g.nodes.append(node("Flatten", [g.pair("g", rng_of(gp))], ["f"], name="flatten", axis=1))
    wd, ws = g.weight("fc.w", w["fc"][0], axis=0)
    bd = g.bias("fc.b", w["fc"][1], g.q["act"].get("g", (None,))[0], ws)
    g.nodes.append(node("Gemm", ["f", wd, bd], ["logits"], name="fc", transB=1))
    out = g.pair("logits", rng_of(y), dequantize=not quantized_output)
    g.q["folded"] = len(g.q["weight"]) + len(g.q["bias"])
    g.q["pairs"] = len(g.q["act"]) - (1 if quantized_output else 0)
    outs = [value_info(out, UINT8 if quantized_output and quantize else FLOAT, ["batch", 5])]
    return model(g.nodes, [value_info("x", FLOAT, ["batch", 3, image, image])], outs, g.inits, opset=19, name="small_cnn_qdq"), g.q


def _np_bert_activations(cfg, w, ids, tts, seq):
    """The f32 encoder in numpy, returning the inputs of its weight MatMuls per layer (calibration only)."""
    import math
    erf = np.vectorize(math.erf)
    H, nh = cfg.hidden, cfg.heads
    dh = H // nh

    def ln(t, gam, bet):
        mu = t.mean(-1, keepdims=True)
        return ((t - mu) / np.sqrt(((t - mu) ** 2).mean(-1, keepdims=True) + cfg.eps) * gam + bet).astype(np.float32)

    x = ln(w["word"][ids] + w["type"][tts] + w["pos"][:seq], w["emb_ln_g"], w["emb_ln_b"])
    acts = []
    for lw in w["layers"]:
        B = x.shape[0]
        split = lambda t: t.reshape(B, seq, nh, dh).transpose(0, 2, 1, 3)
        q, k, v = (split(x @ lw["w" + t] + lw["b" + t]) for t in "qkv")
        sc = q @ k.transpose(0, 1, 3, 2) / np.sqrt(np.float32(dh))
        pr = np.exp(sc - sc.max(-1, keepdims=True))
        pr = pr / pr.sum(-1, keepdims=True)
        ctx = (pr @ v).transpose(0, 2, 1, 3).reshape(B, seq, H)
        x1 = ln(ctx @ lw["wo"] + lw["bo"] + x, lw["ln1_g"], lw["ln1_b"])
        h = x1 @ lw["w1"] + lw["b1"]
        h = (0.5 * h * (1.0 + erf(h / math.sqrt(2.0)))).astype(np.float32)
        x2 = ln(h @ lw["w2"] + lw["b2"] + x1, lw["ln2_g"], lw["ln2_b"])
        acts.append({"x": x, "ctx": ctx, "x1": x1, "h": h})
        x = x2
    return acts


def bert_encoder_qdq(cfg, weights, seq: int, batch="batch", seed: int = 11):
    """bert_encoder after static quantisation of its weight MatMuls in the QDQ layout: i8 weights behind a DequantizeLinear -- per-tensor, the first
    feed-forward weight per column (axis 1) -- and a Q/DQ pair with per-tensor u8 constants on each such MatMul's activation input (the three
    projections share the pair on their input).  The attention products, biases, LayerNormalization and Gelu stay f32.
    -> (model bytes, q) as small_cnn_qdq."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, cfg.vocab, (4, seq))
    acts = _np_bert_activations(cfg, weights, ids, np.zeros((4, seq), np.int64), seq)
    g = _QdqGraph()
    ranges = {}
    for i, a in enumerate(acts):
        x_name = "x0" if i == 0 else f"l{i - 1}.x2"
        ranges.update({x_name: a["x"], f"l{i}.ctx": a["ctx"], f"l{i}.x1": a["x1"], f"l{i}.h": a["h"]})

    def matmul(nodes, inits, x, wname, out, name):
        assert nodes is g.nodes and inits is g.inits
        wd, _ = g.weight(wname, weights["layers"][int(wname[1:wname.index(".")])][wname.split(".")[1]], axis=1 if wname.endswith(".w1") else None)
        t = ranges[x]
        nodes.append(node("MatMul", [g.pair(x, (t.min(), t.max())), wd], [out], name=name))

    data = _bert_encoder(cfg, weights, seq, batch, g.nodes, g.inits, matmul)
    g.q["folded"] = len(g.q["weight"])
    g.q["pairs"] = len(g.q["act"])
    return data, g.q


def resnet50_qdq(weights, batch="batch", image: int = 224, calibration_image: int = 32, quantize: bool = True, seed: int = 13):
    """ResNet-50 (the graph of resnet50_f32) after static quantisation in the QDQ layout, built as small_cnn_qdq: i8 weights per output channel, int32
    biases, a per-tensor u8 Q/DQ pair on the input, behind every Conv(+Add)(+Relu) group, both pools and the logits.  The calibration pass runs the f32
    network in numpy on one seeded `calibration_image`-sized picture (the scales are parameters: any plausible range serves a timing run).
    `quantize=False`: the f32 network written by the same code (output "logits").  -> (model bytes, q)."""
    from .workloads.resnet50 import conv_specs
    specs = conv_specs()
    acts = {"x": np.random.default_rng(seed).random((1, 3, calibration_image, calibration_image), dtype=np.float32)}
    for l in specs:
        t = _np_conv2d(acts[l["src"]], *weights[l["name"]], stride=l["stride"], pad=l["pad"])
        if l["res"]:
            t = t + acts[l["res"]]
        acts[l["dst"]] = np.maximum(t, 0) if l["relu"] else t
        if l["name"] == "stem":
            win = np.lib.stride_tricks.sliding_window_view(np.pad(acts["stem"], ((0, 0), (0, 0), (1, 1), (1, 1)), constant_values=-np.inf), (3, 3), axis=(2, 3))
            acts["pool"] = win[:, :, ::2, ::2].max(axis=(4, 5))
    last = specs[-1]["dst"]
    acts["gap"] = acts[last].mean(axis=(2, 3), keepdims=True)
    fw, fb = weights["fc"]
    acts["logits"] = acts["gap"].reshape(1, -1) @ fw.T + fb
    rng_of = lambda n: (acts[n].min(), acts[n].max())

    g = _QdqGraph(quantize)
    for l in specs:
        n = l["name"]
        xin = g.pair(l["src"], rng_of(l["src"]))
        wd, ws = g.weight(n + ".w", weights[n][0], axis=0)
        bd = g.bias(n + ".b", weights[n][1], g.q["act"].get(l["src"], (None,))[0], ws)
        conv_out = l["dst"] + ".conv" if (l["relu"] or l["res"]) else l["dst"]
        g.nodes.append(node("Conv", [xin, wd, bd], [conv_out], name=n, dilations=[1, 1], group=1, kernel_shape=[l["k"], l["k"]], pads=[l["pad"]] * 4, strides=[l["stride"]] * 2))
        cur = conv_out
        if l["res"]:
            nxt = l["dst"] + ".sum" if l["relu"] else l["dst"]
            g.nodes.append(node("Add", [cur, g.pair(l["res"], rng_of(l["res"]))], [nxt], name=n + ".add"))
            cur = nxt
        if l["relu"]:
            g.nodes.append(node("Relu", [cur], [l["dst"]], name=n + ".relu"))
        if n == "stem":
            g.nodes.append(node("MaxPool", [g.pair("stem", rng_of("stem"))], ["pool"], name="maxpool", ceil_mode=0, kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[2, 2]))
    g.nodes.append(node("GlobalAveragePool", [g.pair(last, rng_of(last))], ["gap"], name="gap"))
    g.nodes.append(node("Flatten", [g.pair("gap", rng_of("gap"))], ["flat"], name="flatten", axis=1))
    wd, ws = g.weight("fc.w", fw, axis=0)
    bd = g.bias("fc.b", fb, g.q["act"].get("gap", (None,))[0], ws)
    g.nodes.append(node("Gemm", ["flat", wd, bd], ["logits"], name="fc", alpha=1.0, beta=1.0, transB=1))
    out = g.pair("logits", rng_of("logits"))
    g.q["folded"] = len(g.q["weight"]) + len(g.q["bias"])
    g.q["pairs"] = len(g.q["act"])
    return model(g.nodes, [value_info("x", FLOAT, [batch, 3, image, image])], [value_info(out, FLOAT, [batch, fw.shape[0]])], g.inits, opset=19, name="resnet50_qdq"), g.q


# ----------------------------------------------------------------------------------------------------------------
# The reduction operators PyTorch's exporter never writes: LpNormalization (both p, a non-last axis), GlobalMaxPool,
# ReduceLogSum, ReduceSumSquare and a Reduce with noop_with_empty_axes = 1.  Opset 18: the axes are constant inputs.
# ----------------------------------------------------------------------------------------------------------------
REDUCE_FAMILY_OUTPUTS = ["lp2_channels", "lp1_last", "global_max", "log_sum", "sum_square", "l1_noop", "log_sum_exp_noop"]


def reduce_family_graph(batch="batch", channels: int = 3, height: int = 5, width: int = 7) -> bytes:
    """x [batch, C, H, W] ->
         lp2_channels      LpNormalization(axis = 1, p = 2)            lanes strided by H * W
         lp1_last          LpNormalization(axis = -1, p = 1)
         global_max        GlobalMaxPool                               [batch, C, 1, 1]
         log_sum           ReduceLogSum(Abs(x) + 1, axes = [2, 3], keepdims = 0)
         sum_square        ReduceSumSquare(axes = [-1], keepdims = 1)
         l1_noop           ReduceL1(noop_with_empty_axes = 1), no axes: |x|
         log_sum_exp_noop  ReduceLogSumExp(noop_with_empty_axes = 1) with an empty axes input: x"""
    i64 = lambda *v: np.array(v, np.int64)
    inits = [tensor("one", np.array(1.0, np.float32)), tensor("axes_hw", i64(2, 3)), tensor("axes_last", i64(-1)), tensor("axes_none", np.zeros(0, np.int64))]
    nodes = [
        node("LpNormalization", ["x"], ["lp2_channels"], name="lp2_channels", axis=1, p=2),
        node("LpNormalization", ["x"], ["lp1_last"], name="lp1_last", axis=-1, p=1),
        node("GlobalMaxPool", ["x"], ["global_max"], name="global_max"),
        node("Abs", ["x"], ["abs_x"], name="abs"),
        node("Add", ["abs_x", "one"], ["positive"], name="add_one"),
        node("ReduceLogSum", ["positive", "axes_hw"], ["log_sum"], name="log_sum", keepdims=0),
        node("ReduceSumSquare", ["x", "axes_last"], ["sum_square"], name="sum_square", keepdims=1),
        node("ReduceL1", ["x"], ["l1_noop"], name="l1_noop", noop_with_empty_axes=1),
        node("ReduceLogSumExp", ["x", "axes_none"], ["log_sum_exp_noop"], name="log_sum_exp_noop", noop_with_empty_axes=1),
    ]
    shape = [batch, channels, height, width]
    outs = [value_info("lp2_channels", FLOAT, shape), value_info("lp1_last", FLOAT, shape), value_info("global_max", FLOAT, [batch, channels, 1, 1]),
            value_info("log_sum", FLOAT, [batch, channels]), value_info("sum_square", FLOAT, [batch, channels, height, 1]), value_info("l1_noop", FLOAT, shape),
            value_info("log_sum_exp_noop", FLOAT, shape)]
    return model(nodes, [value_info("x", FLOAT, shape)], outs, inits, opset=18)


# ----------------------------------------------------------------------------------------------------------------
# Image-to-image graphs: flow warping (GridSample) and sub-pixel super-resolution (DepthToSpace as TensorFlow / Keras
# derived exporters write it; PyTorch's own exporter writes PixelShuffle as Reshape / Transpose / Reshape)
# ----------------------------------------------------------------------------------------------------------------
def base_grid(height: int, width: int, align_corners: bool = False):
    """The identity sampling grid [1, H, W, 2] of GridSample: (x, y) of every output pixel's centre in [-1, 1]."""
    def axis(n):
        i = np.arange(n, dtype=np.float32)
        if align_corners:
            return (i * np.float32(2) / np.float32(max(n - 1, 1)) - np.float32(1)).astype(np.float32)
        return ((i * np.float32(2) + np.float32(1)) / np.float32(n) - np.float32(1)).astype(np.float32)
    gx, gy = np.meshgrid(axis(width), axis(height))
    return np.stack([gx, gy], -1)[None].astype(np.float32)


def flow_warp_graph(seed: int = 21, height: int = 6, width: int = 9, channels: int = 5, align_corners: bool = False, mode: str = "bilinear",
                    padding_mode: str = "zeros", batch="batch"):
    """x [batch, 3, h, w], flow [batch, 2, H, W] (normalised offsets) ->
         feat  Conv 3x3 (3 -> channels), pad 1                                 [batch, channels, h, w]
         grid  Transpose(flow, 0 2 3 1) + the constant identity grid           [batch, H, W, 2]
         warp  GridSample(feat, grid)                                          [batch, channels, H, W]
         y     Conv 1x1 (channels -> 3)
    h and w are free: the sampled plane need not have the grid's size.  Returns (model bytes, weights dict); `mode` / `padding_mode` other than
    the defaults give graphs the loader refuses at the node named "warp"."""
    rng = np.random.default_rng(seed)
    w = {"feat": (rng.normal(0, 0.3, (channels, 3, 3, 3)).astype(np.float32), rng.normal(0, 0.1, channels).astype(np.float32)),
         "out": (rng.normal(0, 0.3, (3, channels, 1, 1)).astype(np.float32), rng.normal(0, 0.1, 3).astype(np.float32)),
         "base_grid": base_grid(height, width, align_corners)}
    inits = [tensor("feat.w", w["feat"][0]), tensor("feat.b", w["feat"][1]), tensor("out.w", w["out"][0]), tensor("out.b", w["out"][1]), tensor("base_grid", w["base_grid"])]
    nodes = [node("Conv", ["x", "feat.w", "feat.b"], ["feat"], name="feat", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
             node("Transpose", ["flow"], ["flow_nhwc"], name="flow_nhwc", perm=[0, 2, 3, 1]),
             node("Add", ["flow_nhwc", "base_grid"], ["grid"], name="grid"),
             node("GridSample", ["feat", "grid"], ["warped"], name="warp", mode=mode, padding_mode=padding_mode, align_corners=int(align_corners)),
             node("Conv", ["warped", "out.w", "out.b"], ["y"], name="out", kernel_shape=[1, 1])]
    ins = [value_info("x", FLOAT, [batch, 3, "h", "w"]), value_info("flow", FLOAT, [batch, 2, height, width])]
    return model(nodes, ins, [value_info("y", FLOAT, [batch, 3, height, width])], inits, opset=16, name="flow_warp"), w


def subpixel_sr_graph(mode: str = "DCR", block: int = 2, seed: int = 23, features: int = 6, batch="batch"):
    """x [batch, 3, h, w] -> Conv 3x3 (3 -> features) -> Relu -> Conv 3x3 (features -> 3 * block^2) -> DepthToSpace(block, mode) [batch, 3, h * block, w * block].
    Returns (model bytes, weights dict).  The weights depend on the seed only, so the DCR and CRD variants (and a PixelShuffle export) can share them."""
    rng = np.random.default_rng(seed)
    w = {"c1": (rng.normal(0, 0.3, (features, 3, 3, 3)).astype(np.float32), rng.normal(0, 0.1, features).astype(np.float32)),
         "c2": (rng.normal(0, 0.2, (3 * block * block, features, 3, 3)).astype(np.float32), rng.normal(0, 0.1, 3 * block * block).astype(np.float32))}
    inits = [tensor("c1.w", w["c1"][0]), tensor("c1.b", w["c1"][1]), tensor("c2.w", w["c2"][0]), tensor("c2.b", w["c2"][1])]
    nodes = [node("Conv", ["x", "c1.w", "c1.b"], ["a"], name="c1", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
             node("Relu", ["a"], ["a.r"], name="c1.relu"),
             node("Conv", ["a.r", "c2.w", "c2.b"], ["b"], name="c2", kernel_shape=[3, 3], pads=[1, 1, 1, 1]),
             node("DepthToSpace", ["b"], ["y"], name="shuffle", blocksize=block, mode=mode)]
    return model(nodes, [value_info("x", FLOAT, [batch, 3, "h", "w"])], [value_info("y", FLOAT, [batch, 3, "H", "W"])], inits, opset=13, name="subpixel_sr"), w


# ----------------------------------------------------------------------------------------------------------------
# CumSum / GatherElements / Trilu / Tile on device data with every attribute (PyTorch's exporter only writes the default forms)
# ----------------------------------------------------------------------------------------------------------------
INDEX_OPS_OUTPUTS = ["cum_excl_rev", "cum_mid_rev", "cum_int_excl", "cum_rows", "gather_mid", "gather_last", "tril_km1", "triu_k1", "tiled"]
INDEX_OPS_BAD = ("cumsum_no_axis", "cumsum_axis_input", "trilu_k_input", "tile_repeats_input", "trilu_extra_input", "tile_extra_input")


def index_ops_graph(batch="batch", rows: int = 4, cols: int = 5, picks: int = 3, bad: str | None = None) -> bytes:
    """x [batch, rows, cols] f32, m [batch, rows, cols] int32, idx [batch, picks, cols] int32 (entries in [-rows, rows)) ->
         cum_excl_rev  CumSum(x, -1, exclusive=1, reverse=1)       cum_mid_rev   CumSum(x, 1, reverse=1)
         cum_int_excl  CumSum(m, 2, exclusive=1)  (int32)          cum_rows      CumSum(x, 0)  (couples the batch rows)
         gather_mid    GatherElements(x, idx, axis=1)              gather_last   GatherElements(x, idx, axis=-1)  (rows <= cols)
         tril_km1      Trilu(x, k=-1, upper=0)                     triu_k1       Trilu(x, k=1)
         tiled         Tile(x, [1, 2, 3])
    `bad` (one of INDEX_OPS_BAD) gives a graph the loader refuses at the node it names: "cum_rows" without its axis operand or with the graph input
    "axis_in" for it, "triu_k1" with the graph input "k_in" / a third input, "tiled" with the graph input "repeats_in" / a third input."""
    assert bad is None or bad in INDEX_OPS_BAD, bad
    shape = [batch, rows, cols]
    i64 = lambda name, v: tensor(name, np.asarray(v, np.int64))
    inits = [i64("axis_m1", -1), i64("axis_0", 0), i64("axis_1", 1), i64("axis_2", 2), i64("k_m1", -1), i64("k_1", 1), i64("repeats", [1, 2, 3])]
    ins = [value_info("x", FLOAT, shape), value_info("m", INT32, shape), value_info("idx", INT32, [batch, picks, cols])]
    cum_rows_in = {"cumsum_no_axis": ["x"], "cumsum_axis_input": ["x", "axis_in"]}.get(bad, ["x", "axis_0"])
    triu_in = {"trilu_k_input": ["x", "k_in"], "trilu_extra_input": ["x", "k_1", "k_m1"]}.get(bad, ["x", "k_1"])
    tile_in = {"tile_repeats_input": ["x", "repeats_in"], "tile_extra_input": ["x", "repeats", "repeats"]}.get(bad, ["x", "repeats"])
    if bad == "cumsum_axis_input":
        ins.append(value_info("axis_in", INT64, []))
    if bad == "trilu_k_input":
        ins.append(value_info("k_in", INT64, []))
    if bad == "tile_repeats_input":
        ins.append(value_info("repeats_in", INT64, [3]))
    nodes = [node("CumSum", ["x", "axis_m1"], ["cum_excl_rev"], name="cum_excl_rev", exclusive=1, reverse=1),
             node("CumSum", ["x", "axis_1"], ["cum_mid_rev"], name="cum_mid_rev", reverse=1),
             node("CumSum", ["m", "axis_2"], ["cum_int_excl"], name="cum_int_excl", exclusive=1),
             node("CumSum", cum_rows_in, ["cum_rows"], name="cum_rows"),
             node("GatherElements", ["x", "idx"], ["gather_mid"], name="gather_mid", axis=1),
             node("GatherElements", ["x", "idx"], ["gather_last"], name="gather_last", axis=-1),
             node("Trilu", ["x", "k_m1"], ["tril_km1"], name="tril_km1", upper=0),
             node("Trilu", triu_in, ["triu_k1"], name="triu_k1"),
             node("Tile", tile_in, ["tiled"], name="tiled")]
    outs = [value_info("cum_excl_rev", FLOAT, shape), value_info("cum_mid_rev", FLOAT, shape), value_info("cum_int_excl", INT32, shape), value_info("cum_rows", FLOAT, shape),
            value_info("gather_mid", FLOAT, [batch, picks, cols]), value_info("gather_last", FLOAT, [batch, picks, cols]), value_info("tril_km1", FLOAT, shape),
            value_info("triu_k1", FLOAT, shape), value_info("tiled", FLOAT, [batch, 2 * rows, 3 * cols])]
    return model(nodes, ins, outs, inits, opset=14, name="index_ops")


# ----------------------------------------------------------------------------------------------------------------
# A detector head that ends in NonMaxSuppression (what an ultralytics export with nms=True, torchvision's detection heads and SSD post-processing end in)
# ----------------------------------------------------------------------------------------------------------------
DETECTOR_HEAD_BAD = ("center_point_box_2", "six_inputs", "max_input", "iou_input", "score_input")


def detector_head_graph(seed: int = 31, features: int = 6, classes: int = 3, batch="batch", center_point_box: int = 0, max_output_boxes_per_class=None,
                        iou_threshold=0.5, score_threshold=None, expose_operands: bool = False, bad: str | None = None):
    """x [batch, features, h, w] -> Conv 1x1 to 4 + classes maps -> Sigmoid -> Split into a box map and a class map -> Reshape / Transpose to
    boxes [batch, h * w, 4] and scores [batch, classes, h * w] -> NonMaxSuppression "nms" with constant scalar operands -> `selected` [count, 3];
    Gather(selected, 2, axis 1) -> the box indices; Gather of image 0's boxes by them -> `picked` [count, 4].  With center_point_box == 0 the far corners
    are moved by +0.6 so that most boxes have a positive area (and some do not).  An optional operand given as None is ABSENT (a later one that is present
    leaves an empty name in its place); max_output_boxes_per_class is an int64 [1] tensor as exporters write it (2 ** 63 - 1 for "all").
    `expose_operands` adds `boxes` and `scores` to the graph outputs.  `bad` (one of DETECTOR_HEAD_BAD) gives a graph the loader refuses at node "nms".
    -> (model bytes, weights)."""
    assert bad is None or bad in DETECTOR_HEAD_BAD, bad
    rng = np.random.default_rng(seed)
    w = {"head": (rng.normal(0, 1.5, (4 + classes, features, 1, 1)).astype(np.float32), rng.normal(0, 0.5, 4 + classes).astype(np.float32))}
    inits = [tensor("head.w", w["head"][0]), tensor("head.b", w["head"][1]), tensor("split_sizes", np.asarray([4, classes], np.int64)),
             tensor("box_shape", np.asarray([0, 4, -1], np.int64)), tensor("cls_shape", np.asarray([0, classes, -1], np.int64)),
             tensor("far_corner_shift", np.asarray([0, 0, 0.6, 0.6], np.float32).reshape(1, 4, 1)), tensor("two", np.asarray(2, np.int64)),
             tensor("zero", np.asarray(0, np.int64))]
    ins = [value_info("x", FLOAT, [batch, features, "h", "w"])]
    scalars = []
    for name, value, dtype, shape in (("max_per_class", max_output_boxes_per_class, np.int64, (1,)), ("iou_thr", iou_threshold, np.float32, (1,)),
                                      ("score_thr", score_threshold, np.float32, ())):
        if bad == {"max_per_class": "max_input", "iou_thr": "iou_input", "score_thr": "score_input"}[name]:
            ins.append(value_info(name + "_in", INT64 if dtype is np.int64 else FLOAT, list(shape)))
            scalars.append(name + "_in")
        elif value is None:
            scalars.append("")
        else:
            inits.append(tensor(name, np.asarray(value, dtype).reshape(shape)))
            scalars.append(name)
    while scalars and scalars[-1] == "":
        scalars.pop()
    if bad == "six_inputs":
        scalars = (scalars + ["", "", ""])[:3] + ["zero"]
    nms_attrs = {"center_point_box": 2 if bad == "center_point_box_2" else center_point_box}
    nodes = [node("Conv", ["x", "head.w", "head.b"], ["head"], name="head", kernel_shape=[1, 1]),
             node("Sigmoid", ["head"], ["head.s"], name="head.sigmoid"),
             node("Split", ["head.s", "split_sizes"], ["box_map", "cls_map"], name="split", axis=1),
             node("Reshape", ["box_map", "box_shape"], ["box_rows"], name="box_rows")]
    if center_point_box == 0:
        nodes.append(node("Add", ["box_rows", "far_corner_shift"], ["box_corners"], name="far_corners"))
    nodes += [node("Transpose", ["box_corners" if center_point_box == 0 else "box_rows"], ["boxes"], name="boxes", perm=[0, 2, 1]),
              node("Reshape", ["cls_map", "cls_shape"], ["scores"], name="scores"),
              node("NonMaxSuppression", ["boxes", "scores"] + scalars, ["selected"], name="nms", **nms_attrs),
              node("Gather", ["selected", "two"], ["box_ids"], name="box_ids", axis=1),
              node("Gather", ["boxes", "zero"], ["boxes0"], name="boxes0", axis=0),
              node("Gather", ["boxes0", "box_ids"], ["picked"], name="picked", axis=0)]
    outs = [value_info("selected", INT64, ["count", 3]), value_info("picked", FLOAT, ["count", 4])]
    if expose_operands:
        outs += [value_info("boxes", FLOAT, [batch, "boxes", 4]), value_info("scores", FLOAT, [batch, classes, "boxes"])]
    return model(nodes, ins, outs, inits, opset=13, name="detector_head"), w


# ----------------------------------------------------------------------------------------------------------------
# Audio front ends: a Whisper-style log-mel spectrogram from the waveform (STFT), and a DFT -> spectral filter -> inverse DFT round trip
# ----------------------------------------------------------------------------------------------------------------
def mel_filterbank(n_fft: int, n_mels: int, sample_rate: float = 16000.0):
    """[n_fft / 2 + 1, n_mels] float32: triangular filters evenly spaced on the HTK mel scale from 0 Hz to sample_rate / 2, each with unit peak."""
    bins = n_fft // 2 + 1
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    edges = hz(np.linspace(mel(0.0), mel(sample_rate / 2.0), n_mels + 2))
    freqs = np.arange(bins) * (sample_rate / n_fft)
    fb = np.zeros((bins, n_mels), np.float64)
    for j in range(n_mels):
        lo, mid, hi = edges[j], edges[j + 1], edges[j + 2]
        fb[:, j] = np.maximum(0.0, np.minimum((freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid)))
    return fb.astype(np.float32)


def hann_window(n: int):
    """torch.hann_window(n) (periodic), float32."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32)


def log_mel_graph(n_fft: int = 400, hop: int = 160, n_mels: int = 80, batch="batch", samples="samples", expose_stft: bool = False):
    """wave [batch, samples] -> reflect Pad of n_fft / 2 on both ends of the sample axis -> STFT "stft" (frame_step = hop, a Hann window initializer, onesided)
    -> re^2 + im^2 -> MatMul with a mel filterbank [bins, n_mels] -> Clip(min 1e-10) -> Log / ln 10 -> Max(l, ReduceMax(l) - 8) -> (l + 4) / 4: the log-mel
    front end of a Whisper-style model, `log_mel` [batch, frames, n_mels].  `expose_stft` adds the STFT node's output `spectrum` [batch, frames, bins, 2] to
    the graph outputs.  -> (model bytes, {"window", "mel"})."""
    w = {"window": hann_window(n_fft), "mel": mel_filterbank(n_fft, n_mels)}
    bins = n_fft // 2 + 1
    inits = [tensor("window", w["window"]), tensor("mel", w["mel"]), tensor("pads", np.asarray([0, n_fft // 2, 0, n_fft // 2], np.int64)),
             tensor("hop", np.asarray(hop, np.int64)), tensor("component_axis", np.asarray([3], np.int64)), tensor("floor", np.asarray(1e-10, np.float32)),
             tensor("inv_ln10", np.asarray(1.0 / np.log(10.0), np.float32)), tensor("eight", np.asarray(8.0, np.float32)), tensor("four", np.asarray(4.0, np.float32))]
    nodes = [node("Pad", ["wave", "pads"], ["padded"], name="center", mode="reflect"),
             node("STFT", ["padded", "hop", "window"], ["spectrum"], name="stft", onesided=1),
             node("Mul", ["spectrum", "spectrum"], ["squares"], name="squares"),
             node("ReduceSum", ["squares", "component_axis"], ["power"], name="power", keepdims=0),
             node("MatMul", ["power", "mel"], ["mel_power"], name="mel"),
             node("Clip", ["mel_power", "floor"], ["clamped"], name="clamp"),
             node("Log", ["clamped"], ["ln"], name="ln"),
             node("Mul", ["ln", "inv_ln10"], ["log10"], name="log10"),
             node("ReduceMax", ["log10"], ["peak"], name="peak", keepdims=1),
             node("Sub", ["peak", "eight"], ["range_floor"], name="range_floor"),
             node("Max", ["log10", "range_floor"], ["floored"], name="floored"),
             node("Add", ["floored", "four"], ["shifted"], name="shift"),
             node("Div", ["shifted", "four"], ["log_mel"], name="scale")]
    outs = [value_info("log_mel", FLOAT, [batch, "frames", n_mels])]
    if expose_stft:
        outs.append(value_info("spectrum", FLOAT, [batch, "frames", bins, 2]))
    return model(nodes, [value_info("wave", FLOAT, [batch, samples])], outs, inits, opset=17, name="log_mel"), w


def dft_graph(opset: int = 17, n: int = 12, dft_length: int | None = None, batch="batch", seed: int = 41):
    """x [batch, n, 1] (real) -> DFT "forward" along the signal axis -> Mul by a real spectral gain [n_fft, 1] -> DFT "inverse" -> `y` [batch, n_fft, 2]; the
    forward spectrum is the second output `spectrum`.  opset 17 writes the axis as the `axis` attribute (1); opset 20 as the third INPUT (-2), the form the
    axis took from opset 20 on.  `dft_length` (a constant second input of the forward node) zero-fills or truncates the signal.  -> (model bytes, {"gain"})."""
    assert opset in (17, 20), opset
    n_fft = n if dft_length is None else dft_length
    rng = np.random.default_rng(seed)
    w = {"gain": rng.uniform(0.25, 1.5, (n_fft, 1)).astype(np.float32)}
    inits = [tensor("gain", w["gain"])]
    length = ""
    if dft_length is not None:
        inits.append(tensor("dft_length", np.asarray(dft_length, np.int64)))
        length = "dft_length"
    if opset == 17:
        fwd_in, inv_in, attrs = ["x"] + ([length] if length else []), ["filtered"], {"axis": 1}
    else:
        inits.append(tensor("axis", np.asarray(-2, np.int64)))
        fwd_in, inv_in, attrs = ["x", length, "axis"], ["filtered", "", "axis"], {}
    nodes = [node("DFT", fwd_in, ["spectrum"], name="forward", **attrs),
             node("Mul", ["spectrum", "gain"], ["filtered"], name="filter"),
             node("DFT", inv_in, ["y"], name="inverse", inverse=1, **attrs)]
    outs = [value_info("y", FLOAT, [batch, n_fft, 2]), value_info("spectrum", FLOAT, [batch, n_fft, 2])]
    return model(nodes, [value_info("x", FLOAT, [batch, n, 1])], outs, inits, opset=opset, name="dft_round_trip"), w


# ----------------------------------------------------------------------------------------------------------------
# Decoder blocks: RMS / skip normalisation and rotary embedding, one graph per operator form, and a genai-builder-style block
# ----------------------------------------------------------------------------------------------------------------
MS = "com.microsoft"
NORM_ROTARY_FORMS = ("rms", "rms_two_axes", "rms_one_element_scale", "simplified", "skip_layer", "skip_layer_plain", "skip_simplified", "skip_simplified_batch_skip",
                     "add_rms", "add_simplified_sole", "rotary", "rotary_ids_4d", "rotary_interleaved_partial", "ms_rotary_offset", "ms_rotary_ids")
NORM_ROTARY_BAD = ("stash_type_0", "skip_mean_read", "skip_inv_std_var_output", "skip_no_epsilon", "rms_int_scale", "rotary_int_cache", "ms_rotary_no_ids")


def rotary_caches(max_pos: int, half: int, base: float = 10000.0):
    """cos / sin caches [max_pos, half] of the usual rotary frequencies, float32."""
    inv = base ** (-np.arange(half, dtype=np.float64) / half)
    ang = np.arange(max_pos, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def norm_rotary_graph(form: str, batch="batch", seq: int = 3, heads: int = 2, head_size: int = 8, max_pos: int = 16, seed: int = 51):
    """One operator form per graph (NORM_ROTARY_FORMS; NORM_ROTARY_BAD are the forms the loader refuses by node name).  The hidden size is heads * head_size.
    Inputs: `x` [batch, seq, hidden] ([batch, heads, seq, head_size] for rotary_ids_4d), `skip` for the skip and Add forms ([1, seq, hidden] for
    skip_simplified_batch_skip), `position_ids` int64 [batch, seq] or `offset` int64 [1] for the position forms.  Outputs: `y`, and `sum` where the form
    exposes the sum.  -> (model bytes, weights)."""
    assert form in NORM_ROTARY_FORMS + NORM_ROTARY_BAD, form
    rng = np.random.default_rng(seed)
    hidden, half = heads * head_size, head_size // 2
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = {"gamma": f(hidden), "beta": f(hidden), "bias": f(hidden), "gamma2": f(seq, hidden), "one": np.asarray([0.75], np.float32)}
    w["cos"], w["sin"] = rotary_caches(max_pos, half)
    w["cos_part"], w["sin_part"] = rotary_caches(max_pos, (head_size - 2) // 2)
    x_info = value_info("x", FLOAT, [batch, seq, hidden])
    skip_info = value_info("skip", FLOAT, [batch, seq, hidden])
    ins, outs, used = [x_info], [value_info("y", FLOAT, [batch, seq, hidden])], []
    sum_info = value_info("sum", FLOAT, [batch, seq, hidden])
    if form in ("rms", "simplified", "stash_type_0", "rms_int_scale"):
        attrs = {"stash_type": 0} if form == "stash_type_0" else {}
        if form == "rms_int_scale":
            w["gamma"] = np.arange(hidden, dtype=np.int32)
        nodes = [node("SimplifiedLayerNormalization" if form == "simplified" else "RMSNormalization", ["x", "gamma"], ["y"], name="norm", axis=-1, epsilon=1e-6, **attrs)]
        used = ["gamma"]
    elif form == "rms_two_axes":
        nodes, used = [node("RMSNormalization", ["x", "gamma2"], ["y"], name="norm", axis=-2)], ["gamma2"]
    elif form == "rms_one_element_scale":
        nodes, used = [node("RMSNormalization", ["x", "one"], ["y"], name="norm")], ["one"]
    elif form in ("skip_layer", "skip_layer_plain", "skip_mean_read", "skip_inv_std_var_output", "skip_no_epsilon"):
        attrs = {} if form == "skip_no_epsilon" else {"epsilon": 1e-5}
        if form == "skip_layer_plain":
            nodes, used = [node("SkipLayerNormalization", ["x", "skip", "gamma"], ["y"], name="skip_norm", domain=MS, **attrs)], ["gamma"]
        else:
            nodes = [node("SkipLayerNormalization", ["x", "skip", "gamma", "beta", "bias"], ["y", "mean", "inv_std_var", "sum"], name="skip_norm", domain=MS, **attrs)]
            used, outs = ["gamma", "beta", "bias"], outs + [sum_info]
        if form == "skip_mean_read":
            nodes.append(node("Identity", ["mean"], ["mean_copy"], name="reads_mean"))
        if form == "skip_inv_std_var_output":
            outs.append(value_info("inv_std_var", FLOAT, []))
        ins.append(skip_info)
    elif form in ("skip_simplified", "skip_simplified_batch_skip"):
        nodes = [node("SkipSimplifiedLayerNormalization", ["x", "skip", "gamma", "bias"], ["y", "", "", "sum"], name="skip_norm", domain=MS, epsilon=1e-6)]
        used, outs = ["gamma", "bias"], outs + [sum_info]
        ins.append(value_info("skip", FLOAT, [1, seq, hidden]) if form == "skip_simplified_batch_skip" else skip_info)
    elif form == "add_rms":  # the residual stream: the sum is read by the normalisation and is a graph output
        nodes = [node("Add", ["x", "skip"], ["sum"], name="residual"), node("RMSNormalization", ["sum", "gamma"], ["y"], name="norm", epsilon=1e-6)]
        used, outs = ["gamma"], outs + [sum_info]
        ins.append(skip_info)
    elif form == "add_simplified_sole":  # the sum has no other reader
        nodes = [node("Add", ["x", "skip"], ["sum"], name="residual"), node("SimplifiedLayerNormalization", ["sum", "gamma"], ["y"], name="norm")]
        used = ["gamma"]
        ins.append(skip_info)
    elif form in ("rotary", "rotary_int_cache"):
        w["cos3"], w["sin3"] = w["cos"][None, :seq], w["sin"][None, :seq]
        if form == "rotary_int_cache":
            w["cos3"] = np.zeros((1, seq, half), np.int32)
        nodes, used = [node("RotaryEmbedding", ["x", "cos3", "sin3"], ["y"], name="rope", num_heads=heads)], ["cos3", "sin3"]
    elif form == "rotary_ids_4d":
        nodes, used = [node("RotaryEmbedding", ["x", "cos", "sin", "position_ids"], ["y"], name="rope")], ["cos", "sin"]
        ins = [value_info("x", FLOAT, [batch, heads, seq, head_size]), value_info("position_ids", INT64, [batch, seq])]
        outs = [value_info("y", FLOAT, [batch, heads, seq, head_size])]
    elif form == "rotary_interleaved_partial":
        nodes = [node("RotaryEmbedding", ["x", "cos_part", "sin_part", "position_ids"], ["y"], name="rope", num_heads=heads, interleaved=1, rotary_embedding_dim=head_size - 2)]
        used = ["cos_part", "sin_part"]
        ins.append(value_info("position_ids", INT64, [batch, seq]))
    elif form == "ms_rotary_offset":
        nodes, used = [node("RotaryEmbedding", ["x", "offset", "cos", "sin"], ["y"], name="rope", domain=MS, num_heads=heads)], ["cos", "sin"]
        ins.append(value_info("offset", INT64, [1]))
    elif form == "ms_rotary_ids":  # num_heads absent: inferred from the cache
        nodes, used = [node("RotaryEmbedding", ["x", "position_ids", "cos", "sin"], ["y"], name="rope", domain=MS)], ["cos", "sin"]
        ins.append(value_info("position_ids", INT64, [batch, seq]))
    else:  # ms_rotary_no_ids
        nodes, used = [node("RotaryEmbedding", ["x", "", "cos", "sin"], ["y"], name="rope", domain=MS, num_heads=heads)], ["cos", "sin"]
    return model(nodes, ins, outs, [tensor(k, w[k]) for k in used], opset=23, name="norm_rotary_" + form), {k: w[k] for k in used}


DECODER_BLOCK_OUTPUTS = ["mlp_out", "residual_out", "present_k", "present_v"]


def decoder_block_graph(hidden: int = 64, heads: int = 4, kv_heads: int = 2, head_size: int = 16, ffn: int = 96, max_pos: int = 32, batch="batch", seq="seq",
                        past="past", seed: int = 61):
    """One decoder block as onnxruntime-genai's builder lays it out, its attention composed from plain operators:
    SkipSimplifiedLayerNormalization(hidden_in, residual_in) -> q / k / v MatMul -> com.microsoft RotaryEmbedding on q and k from the one-element `offset` ->
    head split (Reshape, Transpose) -> Concat with past_k / past_v [batch, kv_heads, past, head_size] (= present_k / present_v) -> KV heads repeated by Unsqueeze,
    Expand, Reshape -> MatMul, Mul by 1 / sqrt(head_size), Softmax, MatMul -> head merge -> output projection -> SkipSimplifiedLayerNormalization with the
    first sum -> gated MLP (gate and up MatMul, Silu, Mul, down MatMul).  Outputs DECODER_BLOCK_OUTPUTS: the MLP output and the second sum (the next block's
    input and skip), present_k, present_v.  -> (model bytes, weights)."""
    assert hidden == heads * head_size and heads % kv_heads == 0
    rng = np.random.default_rng(seed)
    f = lambda *s: (rng.standard_normal(s) / np.sqrt(s[0])).astype(np.float32)
    w = {"ln1_g": (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32), "ln2_g": (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32),
         "wq": f(hidden, heads * head_size), "wk": f(hidden, kv_heads * head_size), "wv": f(hidden, kv_heads * head_size), "wo": f(hidden, hidden),
         "w_gate": f(hidden, ffn), "w_up": f(hidden, ffn), "w_down": f(ffn, hidden)}
    w["cos"], w["sin"] = rotary_caches(max_pos, head_size // 2)
    rep = heads // kv_heads
    i64 = lambda *v: np.asarray(v, np.int64)
    shapes = {"q_split": i64(0, 0, heads, head_size), "kv_split": i64(0, 0, kv_heads, head_size), "rep_axes": i64(2), "rep_shape": i64(1, 1, rep, 1, 1),
              "rep_merge": i64(0, heads, -1, head_size), "merge": i64(0, 0, hidden), "scale": np.asarray(1.0 / np.sqrt(head_size), np.float32)}
    nodes = [node("SkipSimplifiedLayerNormalization", ["hidden_in", "residual_in", "ln1_g"], ["n1", "", "", "res1"], name="input_norm", domain=MS, epsilon=1e-6),
             node("MatMul", ["n1", "wq"], ["q"], name="q_proj"), node("MatMul", ["n1", "wk"], ["k"], name="k_proj"), node("MatMul", ["n1", "wv"], ["v"], name="v_proj"),
             node("RotaryEmbedding", ["q", "offset", "cos", "sin"], ["q_rot"], name="q_rope", domain=MS, num_heads=heads),
             node("RotaryEmbedding", ["k", "offset", "cos", "sin"], ["k_rot"], name="k_rope", domain=MS, num_heads=kv_heads),
             node("Reshape", ["q_rot", "q_split"], ["q4"], name="q_split"), node("Transpose", ["q4"], ["q_heads"], name="q_heads", perm=[0, 2, 1, 3]),
             node("Reshape", ["k_rot", "kv_split"], ["k4"], name="k_split"), node("Transpose", ["k4"], ["k_new"], name="k_heads", perm=[0, 2, 1, 3]),
             node("Reshape", ["v", "kv_split"], ["v4"], name="v_split"), node("Transpose", ["v4"], ["v_new"], name="v_heads", perm=[0, 2, 1, 3]),
             node("Concat", ["past_k", "k_new"], ["present_k"], name="k_cache", axis=2), node("Concat", ["past_v", "v_new"], ["present_v"], name="v_cache", axis=2)]
    for t in ("k", "v"):
        nodes += [node("Unsqueeze", [f"present_{t}", "rep_axes"], [f"{t}_5d"], name=f"{t}_rep_axis"), node("Expand", [f"{t}_5d", "rep_shape"], [f"{t}_rep"], name=f"{t}_repeat"),
                  node("Reshape", [f"{t}_rep", "rep_merge"], [f"{t}_all"], name=f"{t}_rep_merge")]
    nodes += [node("Transpose", ["k_all"], ["k_t"], name="k_transpose", perm=[0, 1, 3, 2]), node("MatMul", ["q_heads", "k_t"], ["scores"], name="qk"),
              node("Mul", ["scores", "scale"], ["scaled"], name="qk_scale"), node("Softmax", ["scaled"], ["probs"], name="softmax", axis=-1),
              node("MatMul", ["probs", "v_all"], ["ctx4"], name="pv"), node("Transpose", ["ctx4"], ["ctx_t"], name="merge_heads", perm=[0, 2, 1, 3]),
              node("Reshape", ["ctx_t", "merge"], ["ctx"], name="merge"), node("MatMul", ["ctx", "wo"], ["attn_out"], name="o_proj"),
              node("SkipSimplifiedLayerNormalization", ["attn_out", "res1", "ln2_g"], ["n2", "", "", "residual_out"], name="post_attention_norm", domain=MS, epsilon=1e-6),
              node("MatMul", ["n2", "w_gate"], ["gate"], name="gate_proj"), node("MatMul", ["n2", "w_up"], ["up"], name="up_proj"),
              node("Silu", ["gate"], ["gate_act"], name="act"), node("Mul", ["gate_act", "up"], ["gated"], name="gated"),
              node("MatMul", ["gated", "w_down"], ["mlp_out"], name="down_proj")]
    ins = [value_info("hidden_in", FLOAT, [batch, seq, hidden]), value_info("residual_in", FLOAT, [batch, seq, hidden]),
           value_info("past_k", FLOAT, [batch, kv_heads, past, head_size]), value_info("past_v", FLOAT, [batch, kv_heads, past, head_size]), value_info("offset", INT64, [1])]
    outs = [value_info("mlp_out", FLOAT, [batch, seq, hidden]), value_info("residual_out", FLOAT, [batch, seq, hidden]),
            value_info("present_k", FLOAT, [batch, kv_heads, "total", head_size]), value_info("present_v", FLOAT, [batch, kv_heads, "total", head_size])]
    inits = [tensor(k, v) for k, v in w.items()] + [tensor(k, v) for k, v in shapes.items()]
    return model(nodes, ins, outs, inits, opset=21, name="decoder_block"), w


GQA_BLOCK_FORMS = ("rotary_nodes", "do_rotary", "packed")


def decoder_block_gqa_graph(form: str = "do_rotary", hidden: int = 64, heads: int = 4, kv_heads: int = 2, head_size: int = 16, ffn: int = 96, max_pos: int = 32,
                            batch="batch", seq="seq", past="past", seed: int = 61, local_window_size: int = -1, **extra_attrs):
    """decoder_block_graph with the same weights and outputs, its attention ONE com.microsoft GroupQueryAttention node, as onnxruntime-genai's builder writes
    it: q / k / v MatMul -> GroupQueryAttention(q, k, v, past_k, past_v, seqlens_k, total_sequence_length[, cos, sin]) -> output projection -> ... (the rest as
    decoder_block_graph).  Forms: "rotary_nodes" -- q and k go through the separate com.microsoft RotaryEmbedding nodes (one-element `offset` input) and
    the node has do_rotary = 0; "do_rotary" -- the node rotates (do_rotary = 1, cos / sin inputs); "packed" -- q, k and v are concatenated into one
    [batch, seq, (heads + 2 kv_heads) * head_size] tensor, key and value are absent, do_rotary = 1.  Inputs: hidden_in, residual_in, past_k, past_v, seqlens_k int32
    [batch], total_sequence_length int32 scalar (and offset).  -> (model bytes, weights)."""
    assert form in GQA_BLOCK_FORMS and hidden == heads * head_size and heads % kv_heads == 0
    rng = np.random.default_rng(seed)
    f = lambda *s: (rng.standard_normal(s) / np.sqrt(s[0])).astype(np.float32)
    w = {"ln1_g": (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32), "ln2_g": (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32),
         "wq": f(hidden, heads * head_size), "wk": f(hidden, kv_heads * head_size), "wv": f(hidden, kv_heads * head_size), "wo": f(hidden, hidden),
         "w_gate": f(hidden, ffn), "w_up": f(hidden, ffn), "w_down": f(ffn, hidden)}
    w["cos"], w["sin"] = rotary_caches(max_pos, head_size // 2)
    nodes = [node("SkipSimplifiedLayerNormalization", ["hidden_in", "residual_in", "ln1_g"], ["n1", "", "", "res1"], name="input_norm", domain=MS, epsilon=1e-6),
             node("MatMul", ["n1", "wq"], ["q"], name="q_proj"), node("MatMul", ["n1", "wk"], ["k"], name="k_proj"), node("MatMul", ["n1", "wv"], ["v"], name="v_proj")]
    attrs = dict(num_heads=heads, kv_num_heads=kv_heads, local_window_size=local_window_size, **extra_attrs)  # extra_attrs: e.g. smooth_softmax=1 for a refusal
    tail = ["past_k", "past_v", "seqlens_k", "total_sequence_length"]
    if form == "rotary_nodes":
        nodes += [node("RotaryEmbedding", ["q", "offset", "cos", "sin"], ["q_rot"], name="q_rope", domain=MS, num_heads=heads),
                  node("RotaryEmbedding", ["k", "offset", "cos", "sin"], ["k_rot"], name="k_rope", domain=MS, num_heads=kv_heads),
                  node("GroupQueryAttention", ["q_rot", "k_rot", "v"] + tail, ["ctx", "present_k", "present_v"], name="attention", domain=MS, **attrs)]
    elif form == "do_rotary":
        nodes += [node("GroupQueryAttention", ["q", "k", "v"] + tail + ["cos", "sin"], ["ctx", "present_k", "present_v"], name="attention", domain=MS, do_rotary=1, **attrs)]
    else:
        nodes += [node("Concat", ["q", "k", "v"], ["qkv"], name="pack_qkv", axis=2),
                  node("GroupQueryAttention", ["qkv", "", ""] + tail + ["cos", "sin"], ["ctx", "present_k", "present_v"], name="attention", domain=MS, do_rotary=1, **attrs)]
    nodes += [node("MatMul", ["ctx", "wo"], ["attn_out"], name="o_proj"),
              node("SkipSimplifiedLayerNormalization", ["attn_out", "res1", "ln2_g"], ["n2", "", "", "residual_out"], name="post_attention_norm", domain=MS, epsilon=1e-6),
              node("MatMul", ["n2", "w_gate"], ["gate"], name="gate_proj"), node("MatMul", ["n2", "w_up"], ["up"], name="up_proj"),
              node("Silu", ["gate"], ["gate_act"], name="act"), node("Mul", ["gate_act", "up"], ["gated"], name="gated"),
              node("MatMul", ["gated", "w_down"], ["mlp_out"], name="down_proj")]
    ins = [value_info("hidden_in", FLOAT, [batch, seq, hidden]), value_info("residual_in", FLOAT, [batch, seq, hidden]),
           value_info("past_k", FLOAT, [batch, kv_heads, past, head_size]), value_info("past_v", FLOAT, [batch, kv_heads, past, head_size]),
           value_info("seqlens_k", INT32, [batch]), value_info("total_sequence_length", INT32, [])]
    if form == "rotary_nodes":
        ins.append(value_info("offset", INT64, [1]))
    outs = [value_info("mlp_out", FLOAT, [batch, seq, hidden]), value_info("residual_out", FLOAT, [batch, seq, hidden]),
            value_info("present_k", FLOAT, [batch, kv_heads, "total", head_size]), value_info("present_v", FLOAT, [batch, kv_heads, "total", head_size])]
    return model(nodes, ins, outs, [tensor(k, v) for k, v in w.items()], opset=21, name="decoder_block_gqa"), w
