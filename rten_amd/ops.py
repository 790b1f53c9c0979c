"""Host-side mirror of RTen's operator interface for the hot path (src/operator.rs:486-613, src/ops/*).

Each class mirrors the reference operator of the same name: same attribute names, same input order,
same validation and the same `OpError` messages (asserted verbatim by the reference's tests, e.g.
src/ops/conv.rs:1182-1268, src/ops/matmul.rs:1284-1333).  Validation runs on the host before any
launch; the arithmetic is done by librten_hip.so through the C ABI (include/rten_hip.h) on
device-resident tensors.  There is no CPU fallback: without the HIP library / an MI355X every `run`
raises.

The Rust reference cannot be compiled in this image (no cargo), so this mirror stands where the Rust
`Operator` impls of INTEGRATION.md would; the registry below mirrors `OpRegistry`
(src/op_registry.rs:25-72).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import lib as L
from .lib import Context
from .tensor import DeviceTensor


class OpError(Exception):
    """Mirrors rten::ops::OpError (src/operator.rs:116-144)."""

    def __init__(self, kind: str, msg: str = ""):
        super().__init__(f"{kind}({msg!r})" if msg else kind)
        self.kind = kind
        self.msg = msg

    def __eq__(self, other):
        return isinstance(other, OpError) and (self.kind, self.msg) == (other.kind, other.msg)

    __hash__ = Exception.__hash__


def InvalidValue(m):
    return OpError("InvalidValue", m)


def IncompatibleInputShapes(m):
    return OpError("IncompatibleInputShapes", m)


def UnsupportedValue(m):
    return OpError("UnsupportedValue", m)


UnsupportedType = OpError("UnsupportedType")
MissingInputs = OpError("MissingInputs")


def _vp(t):
    return None if t is None else C.c_void_p(t.ptr)


def _require(inputs, i):
    if i >= len(inputs) or inputs[i] is None:
        raise MissingInputs
    return inputs[i]


def _get(inputs, i):
    return inputs[i] if i < len(inputs) else None


def _want(t, dtype):
    if t.dtype != np.dtype(dtype):
        raise OpError("InputCastFailed", f"expected {np.dtype(dtype).name} tensor")
    return t


def calc_output_size_and_padding(ctx, in_size, kernel, strides, padding, dilations=(1, 1), ceil_mode=False):
    """src/ops/pooling.rs:139-159 via the C ABI.  padding: "same" or [top, left, bottom, right]."""
    same = isinstance(padding, str)
    if not same and len(padding) != 4:
        raise InvalidValue("Expected 4 padding values")
    pads = (C.c_int32 * 4)(*([0, 0, 0, 0] if same else [int(p) for p in padding]))
    out = (C.c_int32 * 2)()
    opads = (C.c_int32 * 4)()
    msg = C.c_char_p()
    rc = ctx.lib.rten_hip_calc_output_size_and_padding(
        in_size[0], in_size[1], kernel[0], kernel[1], strides[0], strides[1], 1 if same else 0, pads,
        dilations[0], dilations[1], 1 if ceil_mode else 0, out, opads, C.byref(msg))
    if rc:
        raise InvalidValue(msg.value.decode())
    return out[0], out[1], [opads[i] for i in range(4)]


class Operator:
    """Mirror of `trait Operator` (src/operator.rs:486-613): name(), run(ctx, inputs) -> [outputs]."""

    def name(self) -> str:
        return type(self).__name__

    def max_inputs(self):
        return None

    def run(self, ctx: Context, inputs):
        raise NotImplementedError

    # weight staging hook (prepack_inputs / prepack, operator.rs:586-601)
    def prepack_inputs(self):
        return []


# ------------------------------------------------------------------------------------------ Conv
class Conv(Operator):
    """src/ops/conv.rs:367-403.  inputs: X [N,C,H,W] (or [N,C,W]), W [O,C/g,kh,kw], bias [O]?
    Extra (backend fusion of the following graph ops): `fuse_relu`, and a 4th input =
    residual tensor added before the Relu.  `act`: another following activation (an activation operator
    instance such as Sigmoid(), Clip(0, 6), HardSwish()) applied in the epilogue instead; exclusive with fuse_relu."""

    def __init__(self, groups=1, dilations=(1, 1), padding=(0, 0, 0, 0), strides=(1, 1), fuse_relu=False, act=None):
        self.groups = groups
        self.dilations = list(dilations)
        self.padding = padding
        self.strides = list(strides)
        self.fuse_relu = fuse_relu
        self.act = act
        self._packed = {}

    def max_inputs(self):
        return 4

    def prepack_inputs(self):
        return [1]

    def _geometry(self, ctx, xs, ws):
        if len(xs) != 4:
            raise InvalidValue("input must have 4 dims (NCHW)")
        if len(ws) != 4:
            raise InvalidValue("kernel must have 4 dims (OCHW)")
        if len(self.strides) != 2:
            raise InvalidValue("expected 2 stride values")
        if len(self.dilations) != 2:
            raise InvalidValue("expected 2 dilation values")
        n, c, h, w = xs
        o, kc, kh, kw = ws
        oh, ow, pads = calc_output_size_and_padding(ctx, (h, w), (kh, kw), self.strides, self.padding, self.dilations)
        if self.groups == 0:
            raise InvalidValue("Group count must be > 0")
        if c % self.groups != 0:
            raise InvalidValue("Input channel count not divisible by groups")
        if c // self.groups != kc:
            raise IncompatibleInputShapes("Input channels (per group) does not match kernel input channels")
        if o % self.groups != 0:
            raise InvalidValue("Output channel count not divisible by groups")
        d = L.Conv2dDesc(n, c, h, w, o, kh, kw, (C.c_int32 * 4)(*pads), self.strides[0], self.strides[1],
                         self.dilations[0], self.dilations[1], self.groups, oh, ow)
        return d

    def prepack(self, ctx, weight: DeviceTensor, desc=None):
        """Stage weights once (GPU analogue of PrepackedInput, operator.rs:25-66)."""
        if desc is None:
            o, kc, kh, kw = weight.shape
            desc = L.Conv2dDesc(1, kc * self.groups, max(kh, 1), max(kw, 1), o, kh, kw, (C.c_int32 * 4)(0, 0, 0, 0),
                                1, 1, 1, 1, self.groups, 1, 1)
        nbytes = ctx.lib.rten_hip_conv2d_f32_packed_bytes(C.byref(desc))
        packed = DeviceTensor(ctx, (nbytes // 4,), np.float32)
        ctx.call("rten_hip_conv2d_f32_prepack", C.byref(desc), weight.vp, packed.vp)
        return packed

    def _as_2d(self, x, w):
        """1-D convolution: expand to 2-D and remove the extra axis from the result (conv.rs:142-182; views, no copies)."""
        if len(w.shape) != 3:
            raise InvalidValue("kernel must have 3 dims (OCW)")
        if not isinstance(self.padding, str):
            if len(self.padding) != 2:
                raise InvalidValue("expected 2 pad values")
            pad2 = [0, self.padding[0], 0, self.padding[1]]
        else:
            pad2 = "same"
        if len(self.strides) != 1:
            raise InvalidValue("expected 1 stride value")
        if len(self.dilations) != 1:
            raise InvalidValue("expected 1 dilation value")
        op = Conv(self.groups, [1, self.dilations[0]], pad2, [1, self.strides[0]], self.fuse_relu, self.act)
        n, c, wd = x.shape
        return op, x.view((n, c, 1, wd)), w.view((w.shape[0], w.shape[1], 1, w.shape[2]))

    def run(self, ctx, inputs, packed_weight: DeviceTensor | None = None, out: DeviceTensor | None = None):
        x = _want(_require(inputs, 0), np.float32)
        w = _want(_require(inputs, 1), np.float32)
        bias = _get(inputs, 2)
        residual = _get(inputs, 3)
        if len(x.shape) == 3:
            op, x2, w2 = self._as_2d(x, w)
            res2 = residual.view((residual.shape[0], residual.shape[1], 1, residual.shape[2])) if residual is not None else None
            y = op.run(ctx, [x2, w2, bias, res2], packed_weight=packed_weight)[0]
            return [y.view((y.shape[0], y.shape[1], y.shape[3]))]
        d = self._geometry(ctx, x.shape, w.shape)
        if bias is not None and bias.shape[0] != d.o:
            raise IncompatibleInputShapes("bias.size(0) != out_channels")
        y = out if out is not None else DeviceTensor(ctx, (d.n, d.o, d.out_h, d.out_w), np.float32)
        flags = (L.CONV_RELU if self.fuse_relu else 0) | (L.CONV_RESIDUAL if residual is not None else 0)
        wt = packed_weight if packed_weight is not None else w
        if self.act is not None:
            if self.fuse_relu:
                raise InvalidValue("Conv: fuse_relu and act are exclusive")
            kind, alpha, beta = _activation_args(self.act)
            ctx.call("rten_hip_conv2d_f32_act", C.byref(d), x.vp, wt.vp, 1 if packed_weight is not None else 0, _vp(bias),
                     _vp(residual), flags, kind, alpha, beta, y.vp)
        else:
            ctx.call("rten_hip_conv2d_f32", C.byref(d), x.vp, wt.vp, 1 if packed_weight is not None else 0, _vp(bias),
                     _vp(residual), flags, y.vp)
        return [y]


class ConvTranspose(Operator):
    """src/ops/conv_transpose.rs:414-458 (op), :226-412 (conv_transpose).  inputs: X [N,C,H,W] (or [N,C,W]), W [C, O/g, kh, kw], bias [O]?"""

    def __init__(self, padding=(0, 0, 0, 0), groups=1, strides=(1, 1), dilations=(1, 1), output_padding=None):
        self.padding = padding
        self.groups = groups
        self.strides = list(strides)
        self.dilations = list(dilations)
        self.output_padding = None if output_padding is None else list(output_padding)

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        w = _want(_require(inputs, 1), np.float32)
        bias = _get(inputs, 2)
        if len(x.shape) == 3:  # 1-D: expand to 2-D, remove the extra axis from the result (conv_transpose.rs:237-291)
            if len(w.shape) != 3:
                raise InvalidValue("kernel must have 3 dims (OCW)")
            if not isinstance(self.padding, str):
                if len(self.padding) != 2:
                    raise InvalidValue("expected 2 pad values")
                pad2 = [0, self.padding[0], 0, self.padding[1]]
            else:
                pad2 = self.padding
            if len(self.strides) != 1:
                raise InvalidValue("expected 1 stride value")
            if len(self.dilations) != 1:
                raise InvalidValue("expected 1 dilation value")
            if self.output_padding is not None and len(self.output_padding) != 1:
                raise InvalidValue("expected 1 output_padding value")
            op = ConvTranspose(pad2, self.groups, [1, self.strides[0]], [1, self.dilations[0]], [0, self.output_padding[0]] if self.output_padding else None)
            y = op.run(ctx, [x.view((x.shape[0], x.shape[1], 1, x.shape[2])), w.view((w.shape[0], w.shape[1], 1, w.shape[2])), bias])[0]
            return [y.view((y.shape[0], y.shape[1], y.shape[3]))]
        if self.groups == 0:
            raise InvalidValue("Group count must be > 0")
        if len(x.shape) != 4:
            raise InvalidValue("input must have 4 dims (NCHW)")
        if len(w.shape) != 4:
            raise InvalidValue("kernel must have 4 dims (COHW)")
        n, c, h, wd = x.shape
        kc, og, kh, kw = w.shape
        o = og * self.groups
        if bias is not None and bias.shape[0] != o:
            raise IncompatibleInputShapes("bias.size(0) != out_channels")
        if c != kc:
            raise IncompatibleInputShapes("Input channels does not match kernel input channels")
        if kc % self.groups != 0:
            raise InvalidValue("Input channel count not divisible by groups")
        if len(self.strides) != 2:
            raise InvalidValue("expected 2 stride values")
        if len(self.dilations) != 2:
            raise InvalidValue("expected 2 dilation values")
        if self.output_padding is not None and len(self.output_padding) != 2:
            raise InvalidValue("expected 2 output_padding values")
        op_h, op_w = self.output_padding or (0, 0)
        same = isinstance(self.padding, str)
        if not same and len(self.padding) != 4:
            raise InvalidValue("Wrong number of pad values")
        pads = (C.c_int32 * 4)(*([0, 0, 0, 0] if same else [int(p) for p in self.padding]))
        out_hw, out_pads, msg = (C.c_int32 * 2)(), (C.c_int32 * 4)(), C.c_char_p()
        rc = ctx.lib.rten_hip_conv_transpose_output_size(h, wd, kh, kw, self.strides[0], self.strides[1], 1 if same else 0, pads, self.dilations[0], self.dilations[1],
                                                         op_h, op_w, out_hw, out_pads, C.byref(msg))
        if rc:
            raise InvalidValue(msg.value.decode() if msg.value else "")
        d = L.Conv2dDesc(n, c, h, wd, o, kh, kw, out_pads, self.strides[0], self.strides[1], self.dilations[0], self.dilations[1], self.groups, out_hw[0], out_hw[1])
        y = DeviceTensor(ctx, (n, o, out_hw[0], out_hw[1]), np.float32)
        ctx.call("rten_hip_conv_transpose2d_f32", C.byref(d), x.vp, w.vp, _vp(bias), y.vp)
        return [y]


class ConvInteger(Operator):
    """src/ops/conv.rs:478-526.  inputs: X u8|i8, W i8|u8, x_zero_point (scalar)?, w_zero_point (scalar|[O])?"""

    def __init__(self, groups=1, dilations=(1, 1), padding=(0, 0, 0, 0), strides=(1, 1), pad_mode=L.PAD_RAW0_I8):
        self._conv = Conv(groups, dilations, padding, strides)
        self.pad_mode = pad_mode

    def max_inputs(self):
        return 4

    def _desc(self, ctx, x, w, x_zp, w_zp):
        if x.dtype not in (np.uint8, np.int8) or w.dtype not in (np.uint8, np.int8):
            raise UnsupportedType
        o = w.shape[0] if len(w.shape) >= 1 else 0
        if x_zp is not None and x_zp.size != 1:
            raise InvalidValue("input zero point must be a scalar")
        w_zp_len = _zp_len(w_zp, o, "w")  # zero_point_to_vec, matmul.rs:513-531
        d = self._conv._geometry(ctx, x.shape, w.shape)
        return L.Conv2dInt8Desc(d, 1 if x.dtype == np.int8 else 0, 1 if w.dtype == np.int8 else 0, w_zp_len, self.pad_mode)

    def run(self, ctx, inputs, scale=None, bias=None, residual=None, relu=False, out=None):
        x = _require(inputs, 0)
        w = _require(inputs, 1)
        x_zp, w_zp = _get(inputs, 2), _get(inputs, 3)
        di = self._desc(ctx, x, w, x_zp, w_zp)
        d = di.conv
        y = out if out is not None else DeviceTensor(ctx, (d.n, d.o, d.out_h, d.out_w), np.float32 if scale is not None else np.int32)
        flags = (L.CONV_RELU if relu else 0) | (L.CONV_RESIDUAL if residual is not None else 0)
        ctx.call("rten_hip_conv2d_int8", C.byref(di), x.vp, w.vp, _vp(x_zp), _vp(w_zp), _vp(scale), _vp(bias),
                 _vp(residual), flags, y.vp)
        return [y]


class ConvIntegerToFloat(Operator):
    """src/ops/conv.rs:552-587.  inputs: X, W, x_zp, w_zp, scale (scalar).
    Backend fusion extras: bias (the following Add of a [1,O,1,1] constant), residual, relu."""

    def __init__(self, conv: ConvInteger, fuse_relu=False):
        self.conv = conv
        self.fuse_relu = fuse_relu

    def max_inputs(self):
        return 7

    def run(self, ctx, inputs, out=None):
        scale = _want(_require(inputs, 4), np.float32)
        if scale.size != 1:
            raise InvalidValue("scale should be a scalar")
        return self.conv.run(ctx, inputs[:4], scale=scale, bias=_get(inputs, 5), residual=_get(inputs, 6),
                             relu=self.fuse_relu, out=out)


# ------------------------------------------------------------------------------------------ MatMul family
def _broadcast_shapes(a, b):
    try:
        return tuple(np.broadcast_shapes(tuple(a), tuple(b)))
    except ValueError:
        return None


def _matmul(ctx, a: DeviceTensor, b: DeviceTensor, bias=None, alpha=None, act=L.ACT_NONE, b_transposed=False):
    """numpy.matmul rules, src/ops/matmul.rs:208-385.  Contiguous inputs; `b_transposed` reads B as
    [..., N, K] (TransformInputs / transB folded into strides, matmul.rs:47-48, fusions.rs:1066).
    `act`: L.ACT_NONE / ACT_RELU / ACT_GELU, or an activation operator instance (rten_hip_gemm_f32_act)."""
    ext = None
    if act is not None and not isinstance(act, int):
        ext, act = _activation_args(act), L.ACT_NONE
    ash, bsh = list(a.shape), list(b.shape)
    if len(ash) < 1 or len(bsh) < 1:
        raise InvalidValue("Inputs must have >= 1 dimensions")
    a_vec, b_vec = len(ash) == 1, len(bsh) == 1
    if a_vec:
        ash = [1] + ash
    if b_vec:
        bsh = bsh + [1] if not b_transposed else [1] + bsh
    if b_transposed:
        bsh = bsh[:-2] + [bsh[-1], bsh[-2]]
    m, k = ash[-2], ash[-1]
    kb, n = bsh[-2], bsh[-1]
    if k != kb:
        raise IncompatibleInputShapes("Columns of first matrix does not match rows of second matrix")
    pre = _broadcast_shapes(ash[:-2], bsh[:-2])
    if pre is None:
        raise IncompatibleInputShapes("Cannot broadcast shapes")
    out_shape = list(pre) + [m, n]
    na = int(np.prod(ash[:-2], dtype=np.int64))
    nb = int(np.prod(bsh[:-2], dtype=np.int64))
    b_rs, b_cs = (1, k) if b_transposed else (n, 1)
    y = DeviceTensor(ctx, out_shape, np.float32)
    if int(np.prod(out_shape, dtype=np.int64)) > 0:
        if na > 1 and nb == 1:  # matmul.rs:266-297: one [A*M, K] x [K, N] GEMM
            d = L.gemm_desc(na * m, n, k, k, 1, b_rs, b_cs, n, alpha=alpha if alpha is not None else 1.0,
                            bias_kind=L.BIAS_PER_COL if bias is not None else L.BIAS_NONE, act=act)
        else:
            batch = int(np.prod(pre, dtype=np.int64)) if len(pre) else 1
            if na not in (1, batch) or nb not in (1, batch):
                raise UnsupportedValue("partial batch broadcasting is not supported by the device path")
            d = L.gemm_desc(m, n, k, k, 1, b_rs, b_cs, n, batch, m * k if na > 1 else 0, k * n if nb > 1 else 0, m * n,
                            alpha=alpha if alpha is not None else 1.0,
                            bias_kind=L.BIAS_PER_COL if bias is not None else L.BIAS_NONE, act=act)
        if ext is not None:
            ctx.call("rten_hip_gemm_f32_act", C.byref(d), a.vp, b.vp, _vp(bias), ext[0], ext[1], ext[2], y.vp)
        else:
            ctx.call("rten_hip_gemm_f32", C.byref(d), a.vp, b.vp, _vp(bias), y.vp)
    if a_vec:
        out_shape.pop(-2)
    if b_vec:
        out_shape.pop(-1)
    return y.reshape(out_shape) if (a_vec or b_vec) else y


class MatMul(Operator):
    """src/ops/matmul.rs:387-428.  `act` (backend fusion extra): an activation operator instance applied in the epilogue."""

    def __init__(self, act=None):
        self.act = act

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        a = _want(_require(inputs, 0), np.float32)
        b = _want(_require(inputs, 1), np.float32)
        return [_matmul(ctx, a, b, act=self.act if self.act is not None else L.ACT_NONE)]


class FusedMatMul(Operator):
    """src/ops/matmul.rs:455-510: MatMul + bias (per column) + alpha.  `act` is a backend fusion extra
    (GELU epilogue for the BERT FFN): L.ACT_NONE / ACT_RELU / ACT_GELU or an activation operator instance."""

    def __init__(self, alpha=None, act=L.ACT_NONE, transpose_b=False):
        self.alpha = alpha
        self.act = act
        self.transpose_b = transpose_b

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs):
        a = _want(_require(inputs, 0), np.float32)
        b = _want(_require(inputs, 1), np.float32)
        bias = _get(inputs, 2)
        if bias is not None and len(bias.shape) != 1:
            raise OpError("InputCastFailed", "expected tensor with 1 dims")
        return [_matmul(ctx, a, b, bias=bias, alpha=self.alpha, act=self.act, b_transposed=self.transpose_b)]


class Gemm(Operator):
    """src/ops/matmul.rs:106-156: c = alpha * (a b) + beta * c with transA / transB."""

    def __init__(self, alpha=1.0, beta=1.0, transpose_a=False, transpose_b=False):
        self.alpha, self.beta, self.transpose_a, self.transpose_b = alpha, beta, transpose_a, transpose_b

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs):
        a = _want(_require(inputs, 0), np.float32)
        b = _want(_require(inputs, 1), np.float32)
        c = _get(inputs, 2)
        if len(a.shape) != 2:
            raise InvalidValue("a must have 2 dims")
        if len(b.shape) != 2:
            raise InvalidValue("b must have 2 dims")
        m, k = (a.shape[1], a.shape[0]) if self.transpose_a else a.shape
        kb, n = (b.shape[1], b.shape[0]) if self.transpose_b else b.shape
        if k != kb:
            raise IncompatibleInputShapes("Columns of first matrix does not match rows of second matrix")
        a_rs, a_cs = (1, a.shape[1]) if self.transpose_a else (a.shape[1], 1)
        b_rs, b_cs = (1, b.shape[1]) if self.transpose_b else (b.shape[1], 1)
        beta = self.beta if c is not None else 0.0
        if c is not None and beta != 0.0 and _broadcast_shapes(tuple(c.shape), (m, n)) != (m, n):
            raise IncompatibleInputShapes("Cannot broadcast c to output shape")
        y = DeviceTensor(ctx, (m, n), np.float32)
        if c is not None and beta != 0.0:
            # expand_to(c, out_shape) then gemm with beta (matmul.rs:63-82)
            cs = tuple(c.shape)
            if cs == (m, n):
                ctx.call("rten_hip_memcpy_d2d", y.vp, c.vp, C.c_size_t(y.nbytes))
            else:  # row / column / scalar broadcast: materialise via add to zeros
                ctx.call("rten_hip_memset", y.vp, 0, C.c_size_t(y.nbytes))
                if cs in ((n,), (1, n)) or c.size == 1:
                    ctx.call("rten_hip_add_f32", m * n, y.vp, c.vp, c.size, y.vp)
                elif cs == (m, 1):
                    ctx.call("rten_hip_add_channel_bias_f32", 1, m, n, y.vp, c.vp, y.vp)
                else:
                    raise IncompatibleInputShapes("Cannot broadcast c to output shape")
        if m * n > 0:
            d = L.gemm_desc(m, n, k, a_rs, a_cs, b_rs, b_cs, n, alpha=self.alpha, beta=beta)
            ctx.call("rten_hip_gemm_f32", C.byref(d), a.vp, b.vp, None, y.vp)
        return [y]


def _zp_len(zp, expected, what):
    if zp is None:
        return 0
    if len(zp.shape) == 0:
        return 1
    if len(zp.shape) == 1:
        if zp.shape[0] != expected:
            raise InvalidValue("Zero point has incorrect size")
        return expected if expected != 1 else 1
    raise UnsupportedValue("Only scalar or vector zero points are supported")


def _broadcast_prefix(a_prefix, b_prefix):
    """broadcast_shapes (rten-tensor) of two batch prefixes; None when they do not broadcast."""
    n = max(len(a_prefix), len(b_prefix))
    ap = [1] * (n - len(a_prefix)) + list(a_prefix)
    bp = [1] * (n - len(b_prefix)) + list(b_prefix)
    out = []
    for x, y in zip(ap, bp):
        if x != y and x != 1 and y != 1:
            return None
        out.append(max(x, y) if min(x, y) != 0 else 0)
    return out, ap, bp


class MatMulInteger(Operator):
    """src/ops/matmul.rs:582-700 (matmul_integer -> matmul_impl :208-385).  inputs: A u8|i8 [..., M, K], B i8|u8 [..., K, N],
    a_zero_point? (scalar or [M]), b_zero_point? (scalar or [N]).  All of matmul_impl's forms: vector operands, the
    `[A.., M, K] x [K, N]` collapse with the row zero points cycled (:266-280), and batched / broadcast prefixes
    (batched_gemm_uninit, :302-372).  `packed_b`: the RHS staged at load by `prepack` (Operator::prepack, :696-705)."""

    def max_inputs(self):
        return 4

    def prepack_inputs(self):
        return [1]

    def prepack(self, ctx, b):
        """Stage a constant 2-D RHS once (PackedBMatrix).  Returns None when the staged kernel does not cover the shape."""
        if b.dtype not in (np.uint8, np.int8) or len(b.shape) != 2:
            return None
        k, n = b.shape
        nbytes = ctx.lib.rten_hip_gemm_int8_packed_bytes(k, n)
        if not nbytes:
            return None
        packed = DeviceTensor(ctx, [nbytes], np.uint8)
        ctx.call("rten_hip_gemm_int8_prepack", k, n, b.vp, n, 1, 1 if b.dtype == np.int8 else 0, packed.vp)
        packed.packed_for = (k, n, b.dtype)
        return packed

    def run(self, ctx, inputs, scale=None, packed_b=None):
        a = _require(inputs, 0)
        b = _require(inputs, 1)
        if a.dtype not in (np.uint8, np.int8) or b.dtype not in (np.uint8, np.int8):
            raise UnsupportedType
        a_zp, b_zp = _get(inputs, 2), _get(inputs, 3)
        ash, bsh = list(a.shape), list(b.shape)
        a_rows = ash[-2] if len(ash) > 1 else 1  # matmul_integer, matmul.rs:598-607
        b_cols = bsh[-1] if len(bsh) > 1 else 1
        azl = _zp_len(a_zp, a_rows, "a")
        bzl = _zp_len(b_zp, b_cols, "b")
        if len(ash) < 1 or len(bsh) < 1:
            raise InvalidValue("Inputs must have >= 1 dimensions")
        a_is_vec, b_is_vec = len(ash) == 1, len(bsh) == 1  # numpy.matmul rules (matmul.rs:232-240)
        if a_is_vec:
            ash = [1] + ash
        if b_is_vec:
            bsh = bsh + [1]
        m, k = ash[-2], ash[-1]
        kb, n = bsh[-2], bsh[-1]
        if k != kb:
            raise IncompatibleInputShapes("Columns of first matrix does not match rows of second matrix")
        bc = _broadcast_prefix(ash[:-2], bsh[:-2])
        if bc is None:
            raise IncompatibleInputShapes("Cannot broadcast shapes")
        out_prefix, ap, bp = bc
        out_shape = out_prefix + [m, n]
        sl = 0
        if scale is not None:
            if len(scale.shape) > 1:
                raise InvalidValue("scale should have rank 0 or 1")
            sl = 1 if scale.size == 1 else scale.size
            if sl > 1 and sl != n:
                raise IncompatibleInputShapes("Scale length does not match tensor columns")
        final_shape = list(out_shape)
        if a_is_vec:
            del final_shape[-2]
        if b_is_vec:
            del final_shape[-1]
        y = DeviceTensor(ctx, final_shape, np.float32 if scale is not None else np.int32)
        if y.size == 0:
            return [y]
        num_a = int(np.prod(ash[:-2], dtype=np.int64))
        num_b = int(np.prod(bsh[:-2], dtype=np.int64))
        a_s, b_s = 1 if a.dtype == np.int8 else 0, 1 if b.dtype == np.int8 else 0
        use_packed = packed_b is not None and num_b == 1 and getattr(packed_b, "packed_for", None) == (k, n, b.dtype)
        bptr = packed_b.vp if use_packed else b.vp

        def call(mm, a_zp_len, batch, a_bs, b_bs, c_bs, a_off=0, b_off=0, c_off=0):
            d = L.GemmInt8Desc(mm, n, k, k, 1, n, 1, n, a_s, b_s, a_zp_len, bzl, sl, batch, a_bs, b_bs, c_bs, 1 if use_packed else 0)
            itm = y.dtype.itemsize
            ctx.call("rten_hip_gemm_int8", C.byref(d), C.c_void_p(a.ptr + a_off), bptr if use_packed else C.c_void_p(b.ptr + b_off),
                     _vp(a_zp), _vp(b_zp), _vp(scale), C.c_void_p(y.ptr + c_off * itm))

        if num_b == 1:
            # [A.., M, K] x [K, N] as one [A*M, K] x [K, N] product; row r uses a_zp[r % M] (matmul.rs:259-296)
            call(num_a * m, azl, 1, 0, 0, 0)
            return [y]
        # batched products over the broadcast prefix (matmul.rs:302-372)
        nb = int(np.prod(out_prefix, dtype=np.int64))
        if num_a == 1 or ap == out_prefix:
            a_mat = 0 if num_a == 1 else m * k
            if num_b == 1 or bp == out_prefix:
                call(m, azl, nb, a_mat, 0 if num_b == 1 else k * n, m * n)
                return [y]
        # general broadcast: one product per output matrix
        a_str = np.array([0 if d == 1 else int(np.prod(ap[i + 1:], dtype=np.int64)) for i, d in enumerate(ap)], np.int64)
        b_str = np.array([0 if d == 1 else int(np.prod(bp[i + 1:], dtype=np.int64)) for i, d in enumerate(bp)], np.int64)
        for z, idx in enumerate(np.ndindex(*out_prefix)):
            ia, ib = int(np.dot(idx, a_str)), int(np.dot(idx, b_str))
            call(m, azl, 1, 0, 0, 0, a_off=ia * m * k, b_off=ib * k * n, c_off=z * m * n)
        return [y]


class MatMulIntegerToFloat(Operator):
    """src/ops/matmul.rs:775-810.  inputs: A, B, a_zp, b_zp, scale (scalar or [N])."""

    def __init__(self):
        self.matmul = MatMulInteger()

    def max_inputs(self):
        return 5

    def prepack_inputs(self):
        return [1]

    def prepack(self, ctx, b):
        return self.matmul.prepack(ctx, b)

    def run(self, ctx, inputs, packed_b=None):
        scale = _want(_require(inputs, 4), np.float32)
        return self.matmul.run(ctx, inputs[:4], scale=scale, packed_b=packed_b)


class MatMulNBits(Operator):
    """com.microsoft MatMulNBits, src/ops/matmul/contrib.rs:119-196 (op), :21-106 (matmul_nbits).
    inputs: A f32 [..., M, K]; B u8 [N, K/bs, bs/2] (4-bit, even element in the low nibble, zero point 8); scales f32 [N, K/bs] or 1-D.
    accuracy_level 4 (AccuracyLevel::Int8) is an opt-in approximation the reference may decline (contrib.rs:102-108): always Float here."""

    def __init__(self, bits=4, block_size=32, accuracy_level=0):
        self.bits = bits
        self.block_size = block_size
        self.accuracy_level = accuracy_level

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs):
        lhs = _want(_require(inputs, 0), np.float32)
        rhs = _want(_require(inputs, 1), np.uint8)
        if len(rhs.shape) != 3:
            raise OpError("InputCastFailed", "expected tensor with 3 dims")
        scales = _want(_require(inputs, 2), np.float32)
        n = rhs.shape[0]
        if len(scales.shape) == 1:  # earlier versions of the spec used 1-D scales (contrib.rs:152-164)
            k = lhs.shape[-1] if len(lhs.shape) >= 1 else 1
            k_blocks = k // self.block_size if self.block_size else 0
            if scales.size != n * k_blocks:
                raise InvalidValue("Expected 1D `scales` size to match columns * block_size")
        elif len(scales.shape) != 2:
            raise InvalidValue("Expected `scales` to have one or two dims")
        if len(inputs) > 3:
            raise UnsupportedValue("zero_points, g_idx and bias inputs are unsupported")
        if len(lhs.shape) < 2:
            raise InvalidValue("A input must have at least 2 dims")
        if self.bits not in (4, 8):  # BlockQuantizedMatrix::new (block_quant.rs:690-708)
            raise UnsupportedValue("Unsupported bits-per-element")
        bs = rhs.shape[2] * (8 // self.bits)
        if bs < 16 or bs & (bs - 1):
            raise UnsupportedValue("Unsupported K block size")
        rows, k = lhs.shape[-2], lhs.shape[-1]
        if k != rhs.shape[1] * bs:
            raise IncompatibleInputShapes("Columns of first matrix does not match rows of second matrix")
        if self.bits != 4:
            raise UnsupportedValue("MatMulNBits: only 4-bit elements (GemmError::QuantBitsNotSupported, block_quant.rs:77-79)")
        if len(scales.shape) == 2 and tuple(scales.shape) != (n, rhs.shape[1]):
            raise IncompatibleInputShapes("scales shape does not match the quantised matrix")
        batch = int(np.prod(lhs.shape[:-2], dtype=np.int64))
        y = DeviceTensor(ctx, list(lhs.shape[:-1]) + [n], np.float32)
        ctx.call("rten_hip_matmul_nbits_f32", batch, rows, k, n, bs, lhs.vp, rhs.vp, scales.vp, y.vp)
        return [y]


# ------------------------------------------------------------------------------------------ norm / softmax
def _resolve_axis(nd, axis):
    """resolve_axis (src/ops/mod.rs): a rank-0 operand has no valid axis."""
    axis = int(axis)
    if axis < -nd or axis >= nd:
        raise InvalidValue("Axis is invalid")
    return axis + nd if axis < 0 else axis


class Softmax(Operator):
    """src/ops/norm.rs:842-900; any axis (a non-last axis is moved last and back, like normalize_lanes)."""

    def __init__(self, axis=-1, flush_nans_to_zero=False):
        self.axis = axis
        self.flush_nans_to_zero = flush_nans_to_zero

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        nd = len(x.shape)
        ax = _resolve_axis(nd, self.axis)
        flush = 1 if self.flush_nans_to_zero else 0
        if ax != nd - 1:
            # normalize_lanes (src/ops/norm.rs:705-754): move the axis last, make contiguous, apply, move it back
            if nd > 6:
                raise UnsupportedValue("Softmax over a non-last axis of more than 6 dims is not supported by the device path")
            fwd = [i for i in range(nd) if i != ax] + [ax]
            back = [fwd.index(i) for i in range(nd)]
            tshape = [x.shape[i] for i in fwd]
            t, u, y = DeviceTensor(ctx, tshape, np.float32), DeviceTensor(ctx, tshape, np.float32), DeviceTensor(ctx, x.shape, np.float32)
            if x.size:
                cols = x.shape[ax]
                i64 = lambda v: (C.c_int64 * len(v))(*v)
                i32 = lambda v: (C.c_int32 * len(v))(*v)
                ctx.call("rten_hip_transpose_b32", nd, i64(list(x.shape)), i32(fwd), x.vp, t.vp)
                ctx.call("rten_hip_softmax_f32", x.size // cols, cols, t.vp, None, 1, 1, flush, u.vp)
                ctx.call("rten_hip_transpose_b32", nd, i64(tshape), i32(back), u.vp, y.vp)
            return [y]
        y = DeviceTensor(ctx, x.shape, np.float32)
        cols = x.shape[-1]
        ctx.call("rten_hip_softmax_f32", x.size // max(cols, 1), cols, x.vp, None, 1, 1, flush, y.vp)
        return [y]


class AddSoftmax(Operator):
    """src/ops/attention.rs:70-156: Softmax(Add(qk, m), axis=-1); `m` broadcast to qk."""

    def __init__(self, flush_nans_to_zero=False):
        self.flush_nans_to_zero = flush_nans_to_zero

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        y_in = _want(_require(inputs, 1), np.float32)
        qk, m = (x, y_in) if x.size > y_in.size else (y_in, x)
        if _broadcast_shapes(qk.shape, m.shape) != tuple(qk.shape):
            if _broadcast_shapes(qk.shape, m.shape) is None:
                raise IncompatibleInputShapes("Cannot broadcast inputs")
            raise UnsupportedValue("device AddSoftmax needs one input to have the output shape")
        cols = qk.shape[-1]
        rows = qk.size // max(cols, 1)
        msh = (1,) * (len(qk.shape) - len(m.shape)) + tuple(m.shape)
        if msh[-1] != cols:
            raise UnsupportedValue("mask must be contiguous along the softmax axis")
        # Broadcast patterns expressible as addend_row = (row // div) % mod:
        #   same shape; all-ones; prefix [B,1,1] (mask [B,1,1,S] vs scores [B,H,S,S]); suffix [1,1,S].
        # [B,1,S] (prefix + suffix) is run as one launch per leading index.
        lead = msh[:-1]
        qlead = tuple(qk.shape[:-1])
        flush = 1 if self.flush_nans_to_zero else 0
        out = DeviceTensor(ctx, qk.shape, np.float32)

        def prod(t):
            return int(np.prod(t, dtype=np.int64)) if len(t) else 1

        def pattern(ld, ql):
            if ld == ql:
                return 1, max(prod(ql), 1)
            if all(v == 1 for v in ld):
                return max(prod(ql), 1), 1
            i = len(ld)
            while i > 0 and ld[i - 1] == 1:
                i -= 1
            if ld[:i] == ql[:i]:
                return prod(ql[i:]), prod(ql[:i])
            j = 0
            while j < len(ld) and ld[j] == 1:
                j += 1
            if ld[j:] == ql[j:]:
                return 1, prod(ql[j:])
            return None

        pat = pattern(lead, qlead)
        if pat is not None:
            ctx.call("rten_hip_softmax_f32", rows, cols, qk.vp, m.vp, pat[0], pat[1], flush, out.vp)
            return [out]
        if len(lead) >= 2 and lead[0] == qlead[0]:
            sub = pattern(lead[1:], qlead[1:])
            if sub is not None:
                rows_b = prod(qlead[1:])
                m_rows_b = prod(lead[1:])
                for b in range(qlead[0]):
                    ctx.call("rten_hip_softmax_f32", rows_b, cols, C.c_void_p(qk.ptr + b * rows_b * cols * 4),
                             C.c_void_p(m.ptr + b * m_rows_b * cols * 4), sub[0], sub[1], flush,
                             C.c_void_p(out.ptr + b * rows_b * cols * 4))
                return [out]
        raise UnsupportedValue("unsupported mask broadcast pattern on the device path")


class LayerNormalization(Operator):
    """src/ops/norm.rs:531-580.  inputs: X, scale, bias?"""

    def __init__(self, axis=-1, epsilon=None):
        self.axis = axis
        self.epsilon = epsilon

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        scale = _want(_require(inputs, 1), np.float32)
        bias = _get(inputs, 2)
        ax = _resolve_axis(len(x.shape), self.axis)
        norm_shape = tuple(x.shape[ax:])
        cols = int(np.prod(norm_shape, dtype=np.int64))
        gamma = beta = None
        gs, bs = 1.0, 0.0
        if scale.size == 1 and len(scale.shape) == 0:
            gs = float(scale.numpy().reshape(()))
        else:
            if _broadcast_shapes(scale.shape, norm_shape) != norm_shape:
                raise InvalidValue("`scale` is not broadcastable to normalized axes of input")
            if int(np.prod(scale.shape, dtype=np.int64)) != cols:
                raise UnsupportedValue("device path needs scale already expanded to the normalized shape")
            gamma = scale
        if bias is not None:
            if bias.size == 1 and len(bias.shape) == 0:
                bs = float(bias.numpy().reshape(()))
            else:
                if _broadcast_shapes(bias.shape, norm_shape) != norm_shape:
                    raise InvalidValue("`bias` is not broadcastable to normalized axes of input")
                if int(np.prod(bias.shape, dtype=np.int64)) != cols:
                    raise UnsupportedValue("device path needs bias already expanded to the normalized shape")
                beta = bias
        y = DeviceTensor(ctx, x.shape, np.float32)
        eps = 1e-5 if self.epsilon is None else self.epsilon
        ctx.call("rten_hip_layer_norm_f32", x.size // max(cols, 1), cols, x.vp, _vp(gamma), _vp(beta), gs, bs, eps, y.vp)
        return [y]


class BatchNormalization(Operator):
    """src/ops/norm.rs:194-290.  inputs: X, scale, bias, mean, var.  Extra: `act`, an activation operator instance (Relu(), Sigmoid(),
    Clip(0, 6), ...) applied to the result in the same launch (the bits of the two operators in sequence)."""

    def __init__(self, epsilon=1e-5, act=None):
        self.epsilon = epsilon
        self.act = act

    def max_inputs(self):
        return 5

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        scale, bias, mean, var = (_require(inputs, i) for i in range(1, 5))
        if len(x.shape) < 1:
            raise InvalidValue("Input must have at least 1 dim")
        chans = x.shape[1] if len(x.shape) >= 2 else 1
        for t, nm in ((scale, "scale"), (bias, "bias"), (mean, "mean"), (var, "var")):
            if t.shape[0] != chans:
                raise IncompatibleInputShapes(f"{nm}.size(0) != channels")
        n = x.shape[0]
        inner = x.size // max(n * chans, 1)
        y = DeviceTensor(ctx, x.shape, np.float32)
        if self.act is None:
            ctx.call("rten_hip_batch_norm_f32", n, chans, inner, x.vp, scale.vp, bias.vp, mean.vp, var.vp, self.epsilon, y.vp)
        else:
            ctx.call("rten_hip_batch_norm_f32_act", n, chans, inner, x.vp, scale.vp, bias.vp, mean.vp, var.vp, self.epsilon, *_norm_act_args(self.act), y.vp)
        return [y]


def _norm_act_args(act):
    """(kind, alpha, beta) of the `act` of a normalisation operator: None, Relu() / Gelu() or a parameterised activation instance."""
    if act is None:
        return L.ACT_NONE, 0.0, 0.0
    if isinstance(act, Relu):
        return L.ACT_RELU, 0.0, 0.0
    if isinstance(act, Gelu):
        return L.ACT_GELU, 0.0, 0.0
    return _activation_args(act)


class InstanceNormalization(Operator):
    """src/ops/norm.rs:320-395.  inputs: X [N, C, ...], scale [C], bias [C].  epsilon None = the ONNX default 1e-5.  Extra: `act` as for
    BatchNormalization."""

    def __init__(self, epsilon=None, act=None):
        self.epsilon = epsilon
        self.act = act

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs, in_place=False):
        x = _want(_require(inputs, 0), np.float32)
        scale = _want(_require(inputs, 1), np.float32)
        bias = _want(_require(inputs, 2), np.float32)
        if len(x.shape) < 2:
            raise InvalidValue("expected input with >= 2 dims")
        n, chans = x.shape[0], x.shape[1]
        if len(scale.shape) != 1 or scale.shape[0] != chans:
            raise InvalidValue("scale length should match channel count")
        if len(bias.shape) != 1 or bias.shape[0] != chans:
            raise InvalidValue("bias length should match channel count")
        inner = int(np.prod(x.shape[2:], dtype=np.int64))
        eps = 1e-5 if self.epsilon is None else self.epsilon
        y = x if in_place else DeviceTensor(ctx, x.shape, np.float32)
        ctx.call("rten_hip_instance_norm_f32", n, chans, inner, x.vp, scale.vp, bias.vp, eps, *_norm_act_args(self.act), y.vp)
        return [y]


class LogSoftmax(Operator):
    """src/ops/norm.rs:695-800 (log_softmax over normalize_lanes, rten-vecmath/src/softmax.rs:131-174); any axis, a non-last one by the route Softmax takes."""

    def __init__(self, axis=-1):
        self.axis = axis

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        nd = len(x.shape)
        ax = _resolve_axis(nd, self.axis)
        if ax != nd - 1:
            if nd > 6:
                raise UnsupportedValue("LogSoftmax over a non-last axis of more than 6 dims is not supported by the device path")
            fwd = [i for i in range(nd) if i != ax] + [ax]
            back = [fwd.index(i) for i in range(nd)]
            tshape = [x.shape[i] for i in fwd]
            t, y = DeviceTensor(ctx, tshape, np.float32), DeviceTensor(ctx, x.shape, np.float32)
            if x.size:
                cols = x.shape[ax]
                i64 = lambda v: (C.c_int64 * len(v))(*v)
                i32 = lambda v: (C.c_int32 * len(v))(*v)
                ctx.call("rten_hip_transpose_b32", nd, i64(list(x.shape)), i32(fwd), x.vp, t.vp)
                ctx.call("rten_hip_log_softmax_f32", x.size // cols, cols, t.vp, t.vp)  # in place: a wave stores a row only after its last read of it
                ctx.call("rten_hip_transpose_b32", nd, i64(tshape), i32(back), t.vp, y.vp)
            return [y]
        y = DeviceTensor(ctx, x.shape, np.float32)
        cols = x.shape[-1]
        ctx.call("rten_hip_log_softmax_f32", x.size // max(cols, 1), cols, x.vp, y.vp)
        return [y]


# ------------------------------------------------------------------------------------------ elementwise
class _Unary(Operator):
    fn = ""

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs, in_place=False):
        x = _want(_require(inputs, 0), np.float32)
        y = x if in_place else DeviceTensor(ctx, x.shape, np.float32)
        ctx.call(self.fn, x.size, x.vp, y.vp)
        return [y]


class Relu(_Unary):
    """src/ops/unary_elementwise.rs:611-613"""
    fn = "rten_hip_relu_f32"


class Gelu(_Unary):
    """src/ops/unary_elementwise.rs:399-420 (exact erf form)"""
    fn = "rten_hip_gelu_f32"


class Erf(_Unary):
    fn = "rten_hip_erf_f32"


class _Activation(Operator):
    """Element-wise activation with parameters (rten_hip_activation_f32; rten-vecmath/src/exp.rs:201-275, relu.rs:13-25,
    src/ops/unary_elementwise.rs:248-303,437-471).  An instance is also what Conv / MatMul / FusedMatMul take as `act`."""
    kind = L.ACT_NONE

    def __init__(self, alpha=0.0, beta=0.0):
        self.alpha = alpha
        self.beta = beta

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs, in_place=False):
        x = _require(inputs, 0)
        if x.dtype != np.float32:
            raise OpError("UnsupportedType", "expected float32 tensor")
        y = x if in_place else DeviceTensor(ctx, x.shape, np.float32)
        ctx.call("rten_hip_activation_f32", *_activation_args(self), x.size, x.vp, y.vp)
        return [y]


def _activation_args(act):
    """(kind, alpha, beta) of an activation operator instance."""
    if not isinstance(act, _Activation):
        raise InvalidValue(f"expected an activation operator, got {act!r}")
    return act.kind, float(act.alpha), float(act.beta)


class Sigmoid(_Activation):
    kind = L.ACT_SIGMOID


class Silu(_Activation):
    kind = L.ACT_SILU


class Swish(_Activation):
    kind = L.ACT_SWISH

    def __init__(self, alpha=1.0):
        super().__init__(alpha)


class HardSigmoid(_Activation):
    kind = L.ACT_HARD_SIGMOID

    def __init__(self, alpha=0.2, beta=0.5):
        super().__init__(alpha, beta)


class HardSwish(_Activation):
    kind = L.ACT_HARD_SWISH


class LeakyRelu(_Activation):
    kind = L.ACT_LEAKY_RELU

    def __init__(self, alpha=0.01):
        super().__init__(alpha)


class Elu(_Activation):
    kind = L.ACT_ELU

    def __init__(self, alpha=1.0):
        super().__init__(alpha)


F32_MAX = float(np.finfo(np.float32).max)


class Clip(_Activation):
    """Clip(x, min, max) through the reference's Clamp trait: a missing bound is f32::MIN / f32::MAX, NaN becomes min.
    Bounds given as constructor arguments, or as scalar inputs 1 / 2 (read back to the host)."""
    kind = L.ACT_CLIP

    def __init__(self, min=None, max=None):
        super().__init__(-F32_MAX if min is None else min, F32_MAX if max is None else max)

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs, in_place=False):
        lo, hi = _get(inputs, 1), _get(inputs, 2)
        if lo is None and hi is None:
            return super().run(ctx, inputs, in_place)

        def bound(t, dflt):
            if t is None:
                return dflt
            if t.size != 1:
                raise InvalidValue("Clip: min / max must be scalars")
            return float(t.numpy().reshape(-1)[0])
        return Clip(bound(lo, self.alpha), bound(hi, self.beta)).run(ctx, inputs[:1], in_place)


class _Binary(Operator):
    """binary_elementwise.rs:58-170,476-495: numpy broadcasting.  Equal shapes and trailing-dims / per-channel broadcasts take
    the flat 16-byte kernels; anything else goes through the general stride-0 kernel (rten_hip_binary_broadcast_f32)."""
    fn = ""
    opcode = 0
    commutative = True

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs, in_place=False):
        a = _want(_require(inputs, 0), np.float32)
        b = _want(_require(inputs, 1), np.float32)
        if self.commutative and b.size > a.size:  # largest input is the in-place candidate (graph.rs:977-990)
            a, b = b, a
        bshape = _broadcast_shapes(a.shape, b.shape)
        if bshape is None:
            raise IncompatibleInputShapes("Cannot broadcast inputs")
        if bshape == tuple(a.shape):
            bsh = (1,) * (len(a.shape) - len(b.shape)) + tuple(b.shape)
            k = 0
            while k < len(bsh) and bsh[k] == 1:
                k += 1
            if tuple(bsh[k:]) == tuple(a.shape[k:]):  # trailing-dims broadcast (b == a's trailing block)
                y = a if in_place else DeviceTensor(ctx, a.shape, np.float32)
                ctx.call(self.fn, a.size, a.vp, b.vp, b.size, y.vp)
                return [y]
            if self.fn == "rten_hip_add_f32" and len(a.shape) >= 2 and bsh[1] == a.shape[1] and b.size == a.shape[1]:  # [1,C,1,1]
                y = a if in_place else DeviceTensor(ctx, a.shape, np.float32)
                inner = a.size // (a.shape[0] * a.shape[1])
                ctx.call("rten_hip_add_channel_bias_f32", a.shape[0], a.shape[1], inner, a.vp, b.vp, y.vp)
                return [y]
        nd = len(bshape)
        if nd > 6:
            raise UnsupportedValue("broadcasting over more than 6 dims is not supported by the device path")

        def strides(shape):
            sh, st, acc = (1,) * (nd - len(shape)) + tuple(shape), [0] * nd, 1
            for i in range(nd - 1, -1, -1):
                st[i] = 0 if sh[i] == 1 else acc
                acc *= sh[i]
            return st
        y = DeviceTensor(ctx, bshape, np.float32)
        i64 = lambda v: (C.c_int64 * max(len(v), 1))(*v)
        if y.size:
            ctx.call("rten_hip_binary_broadcast_f32", self.opcode, nd, i64(list(bshape)), i64(strides(a.shape)), i64(strides(b.shape)), a.vp, b.vp, y.vp)
        return [y]


class Add(_Binary):
    """src/ops/binary_elementwise.rs:476-495"""
    fn, opcode = "rten_hip_add_f32", 0


class Mul(_Binary):
    fn, opcode = "rten_hip_mul_f32", 1


class Sub(_Binary):
    fn, opcode, commutative = "rten_hip_sub_f32", 2, False


class Div(_Binary):
    """binary_elementwise.rs:613-637: a divisor of exactly one element, at any rank, is multiplied by its reciprocal -- a * (1 / b), two roundings --
    and every other divisor is a true division (`divide`)."""
    fn, opcode, commutative = "rten_hip_div_f32", 3, False

    def run(self, ctx, inputs, in_place=False):
        a = _want(_require(inputs, 0), np.float32)
        b = _want(_require(inputs, 1), np.float32)
        if b.size != 1:
            return self.divide(ctx, inputs, in_place)
        r = DeviceTensor(ctx, b.shape, np.float32)
        ctx.call("rten_hip_unary_f32", L.UNARY_RECIPROCAL, 1, b.vp, r.vp)
        return Mul().run(ctx, [a, r], in_place)

    def divide(self, ctx, inputs, in_place=False):
        return super().run(ctx, inputs, in_place)


# ------------------------------------------------------------------------------------------ unary math, Pow, PRelu, variadic, Pad
def _i64(v):
    return (C.c_int64 * max(len(v), 1))(*[int(a) for a in v])


class _UnaryMath(Operator):
    """src/ops/unary_elementwise.rs: float32 through rten_hip_unary_f32 (one kernel instantiation per operator); the operators the reference also
    defines for int32 (Neg, Abs, Sign) through an RTEN_HIP_EW_* code of rten_hip_elementwise_nd."""
    code = -1
    int_code = None

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs, in_place=False):
        x = _require(inputs, 0)
        if x.dtype == np.int32 and self.int_code is not None:
            y = x if in_place else DeviceTensor(ctx, x.shape, np.int32)
            if x.size:
                ctx.call("rten_hip_elementwise_nd", self.int_code, 1, _i64([x.size]), x.vp, L.DT_I32, _i64([1]), None, L.DT_I32, None, None, None, y.vp, L.DT_I32)
            return [y]
        if self.int_code is not None and x.dtype != np.float32:
            raise UnsupportedType
        _want(x, np.float32)
        y = x if in_place else DeviceTensor(ctx, x.shape, np.float32)
        ctx.call("rten_hip_unary_f32", self.code, x.size, x.vp, y.vp)
        return [y]


class Neg(_UnaryMath):
    code, int_code = L.UNARY_NEG, L.EW_INEG


class Abs(_UnaryMath):
    code, int_code = L.UNARY_ABS, L.EW_IABS


class Sign(_UnaryMath):
    """Rust signum: +0 -> 1, -0 -> -1, NaN -> NaN (float32); -1 / 0 / 1 (int32)."""
    code, int_code = L.UNARY_SIGN, L.EW_ISIGN


class Floor(_UnaryMath):
    code = L.UNARY_FLOOR


class Ceil(_UnaryMath):
    code = L.UNARY_CEIL


class Round(_UnaryMath):
    """round_ties_even"""
    code = L.UNARY_ROUND


class Sqrt(_UnaryMath):
    code = L.UNARY_SQRT


class Reciprocal(_UnaryMath):
    code = L.UNARY_RECIPROCAL


class Exp(_UnaryMath):
    """rten-vecmath/src/exp.rs:59-132, bit-identical"""
    code = L.UNARY_EXP


class Log(_UnaryMath):
    """The float64 logarithm rounded once (the reference calls the host's logf: docs/KERNELS.md 4.8)."""
    code = L.UNARY_LOG


class Softplus(_UnaryMath):
    """exp(x).ln_1p() with exp(x) rounded to float32, each step the float64 function rounded once."""
    code = L.UNARY_SOFTPLUS


def _expanded_strides(shape, nd):
    sh, st, acc = (1,) * (nd - len(shape)) + tuple(shape), [0] * nd, 1
    for i in range(nd - 1, -1, -1):
        st[i] = 0 if sh[i] == 1 else acc
        acc *= sh[i]
    return st


def _broadcast_launch(ctx, a, b, f32_op, i32_op):
    """y = op(a, b) with numpy broadcasting, operand order kept: float32 through rten_hip_binary_broadcast_f32 (`f32_op`), int32 through
    rten_hip_elementwise_nd (`i32_op`)."""
    bshape = _broadcast_shapes(a.shape, b.shape)
    if bshape is None:
        raise IncompatibleInputShapes("Cannot broadcast inputs")
    nd = len(bshape)
    if nd > 6:
        raise UnsupportedValue("broadcasting over more than 6 dims is not supported by the device path")
    y = DeviceTensor(ctx, bshape, a.dtype)
    if y.size:
        sa, sb = _i64(_expanded_strides(a.shape, nd)), _i64(_expanded_strides(b.shape, nd))
        if a.dtype == np.float32:
            ctx.call("rten_hip_binary_broadcast_f32", f32_op, nd, _i64(list(bshape)), sa, sb, a.vp, b.vp, y.vp)
        else:
            ctx.call("rten_hip_elementwise_nd", i32_op, nd, _i64(list(bshape)), a.vp, L.DT_I32, sa, b.vp, L.DT_I32, sb, None, None, y.vp, L.DT_I32)
    return y


class Pow(Operator):
    """src/ops/binary_elementwise.rs:958-1117, float32 base and exponent: exponent 2 -> x * x, 3 -> x * x * x (tested per element), otherwise the
    float64 pow rounded once.  The reference's int32-base forms are not built."""

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        base, exponent = _require(inputs, 0), _require(inputs, 1)
        if base.dtype == np.int32 and exponent.dtype in (np.dtype(np.float32), np.dtype(np.int32)):
            raise UnsupportedValue("Pow: int32 base is not supported by the device path")
        if base.dtype != np.float32 or exponent.dtype != np.float32:
            raise UnsupportedValue("Unsupported base and exponent type combination")
        return [_broadcast_launch(ctx, base, exponent, L.BINARY_POW, None)]


class PRelu(Operator):
    """src/ops/unary_elementwise.rs:624-671: x < 0 ? slope * x : x; the slope broadcasts to x's shape only."""

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        if x.dtype != np.float32:
            raise UnsupportedType
        slope = _want(_require(inputs, 1), np.float32)
        if _broadcast_shapes(x.shape, slope.shape) != tuple(x.shape):
            raise IncompatibleInputShapes("Slope is not broadcastable to input shape")
        return [_broadcast_launch(ctx, x, slope, L.BINARY_PRELU, None)]


class _Variadic(Operator):
    """src/ops/variadic_elementwise.rs:21-39: one input is a copy, otherwise a left fold of the binary operator with numpy broadcasting."""
    f32_op, i32_op = None, None

    def _operands(self, inputs):
        first = _require(inputs, 0)
        if first.dtype not in (np.dtype(np.float32), np.dtype(np.int32)):
            raise UnsupportedType
        return [_want(t, first.dtype) for t in inputs if t is not None]

    def run(self, ctx, inputs):
        ts = self._operands(inputs)
        if len(ts) == 1:
            y = DeviceTensor(ctx, ts[0].shape, ts[0].dtype)
            if y.nbytes:
                ctx.call("rten_hip_memcpy_d2d", y.vp, ts[0].vp, C.c_size_t(y.nbytes))
            return [y]
        acc = ts[0]
        for b in ts[1:]:
            acc = _broadcast_launch(ctx, acc, b, self.f32_op, self.i32_op)
        return [acc]


class Min(_Variadic):
    """cmp_nan_less (reduce.rs:861-873): a NaN in either operand wins, a tie keeps the left operand."""
    f32_op, i32_op = L.BINARY_MIN, L.EW_IMIN


class Max(_Variadic):
    """cmp_nan_greater (reduce.rs:847-859): a NaN in either operand wins, a tie keeps the left operand (Max(+0, -0) = +0, Max(-0, +0) = -0)."""
    f32_op, i32_op = L.BINARY_MAX, L.EW_IMAX


class Sum(_Variadic):
    """Left fold of `+` (int32 wraps)."""
    f32_op, i32_op = L.BINARY_ADD, L.EW_IADD


class Mean(_Variadic):
    """Sum, then divided by n as f32 (variadic_elementwise.rs:98-102: x / n, a true division -- not the Div operator's reciprocal rule)."""
    f32_op = L.BINARY_ADD

    def run(self, ctx, inputs):
        first = _want(_require(inputs, 0), np.float32)
        ts = self._operands(inputs)
        total = super().run(ctx, [first] + ts[1:])[0]
        return Div().divide(ctx, [total, DeviceTensor.from_numpy(ctx, np.float32(len(ts)))], in_place=True)


PAD_MODES = {"constant": L.PAD_CONSTANT, "reflect": L.PAD_REFLECT, "edge": L.PAD_EDGE, "wrap": L.PAD_WRAP}


def pad_geometry(shape, pads, mode):
    """The reference's checks (src/ops/pad.rs:41-124) on a shape: returns (output shape, whether the result is a plain copy of the cropped input)."""
    nd = len(shape)
    if len(pads) != 2 * nd:
        raise InvalidValue("padding length should be 2 * input dims")
    cropped = list(shape)
    if any(p < 0 for p in pads):
        for d in range(nd):
            crop = max(-pads[d], 0) + max(-pads[nd + d], 0)
            if crop > shape[d]:
                raise InvalidValue("Negative pads remove more elements than axis contains")
            cropped[d] = shape[d] - crop
    out = [max(pads[d], 0) + cropped[d] + max(pads[nd + d], 0) for d in range(nd)]
    if out == cropped:
        return out, True
    if mode != "constant":
        batch = max(nd - 2, 0)
        if out[:batch] != cropped[:batch]:
            raise UnsupportedValue("Pad only supports non-constant padding of last 2 dims")
        if 0 in cropped[batch:]:
            raise InvalidValue("Padded dimension for non-constant padding is empty")
    return out, False


class Pad(Operator):
    """src/ops/pad.rs: inputs (data, pads, constant_value, axes); float32 / int32 data of at most 6 dims.  `pads` is a host-side operand (a numpy
    array or list, or a DeviceTensor that is read back), the fill value a scalar of the data's type.  One launch, rten_hip_pad_b32."""

    def __init__(self, mode="constant"):
        if mode not in PAD_MODES:
            raise InvalidValue(f"Pad: unknown mode {mode!r}")
        self.mode = mode

    def max_inputs(self):
        return 4

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        pads_t = _require(inputs, 1)
        if _get(inputs, 3) is not None:
            raise UnsupportedValue("Pad operator does not yet support `axes` input")
        if x.dtype not in (np.dtype(np.float32), np.dtype(np.int32)):
            raise UnsupportedType
        pads_a = _host_values(pads_t)
        if pads_a.ndim != 1:
            raise OpError("InputCastFailed", "expected pads with 1 dims")
        pads = [int(p) for p in pads_a]
        value = _get(inputs, 2)
        fill = np.zeros((), x.dtype)
        if value is not None:
            if value.dtype != x.dtype:
                raise OpError("InputCastFailed", f"expected {x.dtype.name} tensor")
            if len(value.shape) != 0:
                raise OpError("InputCastFailed", "expected tensor with 0 dims")
            fill = np.asarray(_host_values(value), x.dtype).reshape(())
        out, _ = pad_geometry(list(x.shape), pads, self.mode)
        if len(x.shape) > 6:
            raise UnsupportedValue("Pad of more than 6 dims is not supported by the device path")
        y = DeviceTensor(ctx, out, x.dtype)
        if y.size:
            ctx.call("rten_hip_pad_b32", PAD_MODES[self.mode], len(x.shape), _i64(list(x.shape)), _i64(pads), C.c_uint32(int(fill.view(np.uint32))), x.vp, y.vp)
        return [y]


class Transpose(Operator):
    """src/ops/layout.rs:669+: perm None = reverse the axes; 4-byte element types."""

    def __init__(self, perm=None):
        self.perm = perm

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        if x.dtype.itemsize != 4:
            raise UnsupportedType
        nd = len(x.shape)
        perm = list(range(nd - 1, -1, -1)) if self.perm is None else [p + nd if p < 0 else p for p in self.perm]
        if sorted(perm) != list(range(nd)):
            raise InvalidValue("Permutation is invalid")
        y = DeviceTensor(ctx, [x.shape[p] for p in perm], x.dtype)
        if nd > 6:
            raise UnsupportedValue("transpose of more than 6 dims is not supported by the device path")
        ctx.call("rten_hip_transpose_b32", nd, (C.c_int64 * max(nd, 1))(*x.shape), (C.c_int32 * max(nd, 1))(*perm), x.vp, y.vp)
        return [y]


# ------------------------------------------------------------------------------------------ pooling
class _Pool(Operator):
    fn = ""

    def __init__(self, kernel_size, padding=(0, 0, 0, 0), strides=None, ceil_mode=False, count_include_pad=False):
        self.kernel_size = list(kernel_size)
        self.padding = padding
        self.strides = list(strides) if strides is not None else [1] * len(self.kernel_size)
        self.ceil_mode = ceil_mode
        self.count_include_pad = count_include_pad

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        spatial = max(len(x.shape) - 2, 0)
        if len(self.kernel_size) != spatial:
            raise InvalidValue("kernel_size len does not match spatial dims")
        if len(self.strides) != spatial:
            raise InvalidValue("strides len does not match spatial dims")
        if spatial != 2:
            raise UnsupportedValue("Only inputs with 1 or 2 spatial dims are supported")
        n, c, h, w = x.shape
        oh, ow, pads = calc_output_size_and_padding(ctx, (h, w), self.kernel_size, self.strides, self.padding, (1, 1), self.ceil_mode)
        d = L.Pool2dDesc(n, c, h, w, self.kernel_size[0], self.kernel_size[1], self.strides[0], self.strides[1],
                         (C.c_int32 * 4)(*pads), oh, ow, 1 if self.count_include_pad else 0)
        y = DeviceTensor(ctx, (n, c, oh, ow), np.float32)
        ctx.call(self.fn, C.byref(d), x.vp, y.vp)
        return [y]


class MaxPool(_Pool):
    """src/ops/pooling.rs:602-660"""
    fn = "rten_hip_max_pool2d_f32"


class AveragePool(_Pool):
    """src/ops/pooling.rs:419-475"""
    fn = "rten_hip_average_pool2d_f32"


class GlobalAveragePool(Operator):
    """src/ops/pooling.rs:516-545"""

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        if len(x.shape) < 2:
            raise InvalidValue("Input must have at least 2 dims")
        n, c = x.shape[:2]
        inner = x.size // max(n * c, 1)
        y = DeviceTensor(ctx, (n, c) + (1,) * (len(x.shape) - 2), np.float32)
        ctx.call("rten_hip_global_average_pool_f32", n * c, inner, x.vp, y.vp)
        return [y]


class Flatten(Operator):
    """src/ops/layout.rs:264: zero-copy view on device."""

    def __init__(self, axis=1):
        self.axis = axis

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        ax = _resolve_axis(len(x.shape) + 1, self.axis) if self.axis != len(x.shape) else self.axis
        outer = int(np.prod(x.shape[:ax], dtype=np.int64))
        return [x.reshape(outer, -1)]


# ------------------------------------------------------------------------------------------ quantization
class DynamicQuantizeLinear(Operator):
    """src/ops/quantize.rs:438-478 -> [y u8, y_scale f32 scalar, y_zero_point u8 scalar] (all on device)."""

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        y = DeviceTensor(ctx, x.shape, np.uint8)
        scale = DeviceTensor(ctx, (), np.float32)
        zp = DeviceTensor(ctx, (), np.uint8)
        ctx.call("rten_hip_dynamic_quantize_linear", x.size, x.vp, y.vp, scale.vp, zp.vp)
        return [y, scale, zp]


_QDQ_DT = {np.dtype(np.uint8): L.DT_U8, np.dtype(np.int8): L.DT_I8, np.dtype(np.int32): L.DT_I32}


def _qdq_geometry(x, scale, zero_point, axis, what):
    """quantize.rs:41-99,196-275: a scalar or one-element scale is per-tensor (its zero point must have one element); a rank-1 scale is per-axis and is
    checked against the axis; anything else is blocked quantisation.  -> (outer, channels, inner).  One deviation: the reference does not check the
    zero-point length of a per-axis QuantizeLinear (its zip is cut short); a mismatch is refused here with DequantizeLinear's message."""
    if scale.size == 1:
        if zero_point is not None and zero_point.size != 1:
            raise InvalidValue("scale and zero_point must have same shape")
        return 1, 1, int(x.size)
    if len(scale.shape) != 1:
        raise UnsupportedValue(f"Blocked {what} is not supported")
    ax = _resolve_axis(len(x.shape), axis)
    if scale.shape[0] != x.shape[ax]:
        raise IncompatibleInputShapes("scale length does not match size of quantization axis")
    if zero_point is not None:
        if len(zero_point.shape) != 1:
            raise InvalidValue("scale and zero point must have same rank" if what == "dequantization" else "scale and zero point must have same shape")
        if zero_point.shape[0] != x.shape[ax]:
            raise IncompatibleInputShapes("zero_point length does not match size of quantization axis")
    return int(np.prod(x.shape[:ax], dtype=np.int64)), int(x.shape[ax]), int(np.prod(x.shape[ax + 1:], dtype=np.int64))


class QuantizeLinear(Operator):
    """src/ops/quantize.rs:196-334.  Inputs (x f32, y_scale f32, y_zero_point u8 / i8, optional); the output type is the zero point's, or
    `output_dtype` (np.uint8 / np.int8) without one.  scale and zero point stay on the device: nothing is read back."""

    def __init__(self, axis=-1, output_dtype=None):
        self.axis = axis
        self.output_dtype = None if output_dtype is None else np.dtype(output_dtype)

    def max_inputs(self):
        return 3

    def out_dtype(self, zero_point):
        u8, i8 = np.dtype(np.uint8), np.dtype(np.int8)
        if zero_point is not None:
            if zero_point.dtype in (u8, i8) and self.output_dtype in (None, zero_point.dtype):
                return zero_point.dtype
        elif self.output_dtype in (u8, i8):
            return self.output_dtype
        raise UnsupportedType

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        scale = _want(_require(inputs, 1), np.float32)
        zp = _get(inputs, 2)
        dt = self.out_dtype(zp)
        outer, channels, inner = _qdq_geometry(x, scale, zp, self.axis, "quantization")
        y = DeviceTensor(ctx, x.shape, dt)
        if x.size:
            ctx.call("rten_hip_quantize_linear_f32", _QDQ_DT[dt], outer, channels, inner, x.vp, scale.vp, _vp(zp), y.vp)
        return [y]


class DequantizeLinear(Operator):
    """src/ops/quantize.rs:41-133.  Inputs (x u8 / i8 / i32, x_scale f32, x_zero_point of x's type, optional) -> f32."""

    def __init__(self, axis=1):
        self.axis = axis

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        scale = _want(_require(inputs, 1), np.float32)
        if x.dtype not in _QDQ_DT:
            raise UnsupportedType
        zp = _get(inputs, 2)
        if zp is not None:
            _want(zp, x.dtype)
        outer, channels, inner = _qdq_geometry(x, scale, zp, self.axis, "dequantization")
        y = DeviceTensor(ctx, x.shape, np.float32)
        if x.size:
            ctx.call("rten_hip_dequantize_linear_f32", _QDQ_DT[x.dtype], outer, channels, inner, x.vp, scale.vp, _vp(zp), y.vp)
        return [y]


# ------------------------------------------------------------------------------------------ attention
class Attention(Operator):
    """ONNX Attention restricted to the BERT path (src/ops/attention.rs:645-905): 4-D Q/K/V
    [B,H,S,D], optional additive float mask [B,1,1,T] or [B,1,S,T]; no KV cache / GQA / causal."""

    def __init__(self, scale=None):
        self.scale = scale

    def max_inputs(self):
        return 4

    def run(self, ctx, inputs):
        q = _want(_require(inputs, 0), np.float32)
        k = _want(_require(inputs, 1), np.float32)
        v = _want(_require(inputs, 2), np.float32)
        mask = _get(inputs, 3)
        if len(q.shape) != 4 or len(k.shape) != 4 or len(v.shape) != 4:
            raise UnsupportedValue("device Attention needs 4-D Q/K/V")
        B, H, S, D = q.shape
        T, Dv = k.shape[2], v.shape[3]
        if k.shape[:2] != (B, H) or v.shape[:3] != (B, H, T) or k.shape[3] != D:
            raise IncompatibleInputShapes("Q/K/V shapes are inconsistent")
        # `1.0 / (head_size as f32).sqrt()` in f32 arithmetic (attention.rs:659-670)
        scale = self.scale if self.scale is not None else float(np.float32(1.0) / np.sqrt(np.float32(D)))
        mbs, mrs = 0, 0
        if mask is not None:
            if mask.dtype != np.float32:
                raise UnsupportedValue("device Attention supports additive float masks")
            if tuple(mask.shape) == (B, 1, 1, T):
                mbs, mrs = T, 0
            elif tuple(mask.shape) == (B, 1, S, T):
                mbs, mrs = S * T, T
            else:
                raise UnsupportedValue("mask must be [B,1,1,T] or [B,1,S,T]")
        out = DeviceTensor(ctx, (B, H, S, Dv), np.float32)
        d = L.SdpaDesc(B, H, S, T, D, Dv, H * S * D, S * D, D, H * T * D, T * D, D, H * T * Dv, T * Dv, Dv,
                       H * S * Dv, S * Dv, Dv, mbs, mrs, scale, 1)
        ctx.call("rten_hip_sdpa_f32", C.byref(d), q.vp, k.vp, v.vp, _vp(mask), out.vp)
        return [out]


class Gather(Operator):
    """Gather along axis 0 of a 2-D f32 table (embedding lookup; src/ops/gather.rs).  inputs: table [R,W], ids i32."""

    def __init__(self, axis=0):
        self.axis = axis

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        table = _want(_require(inputs, 0), np.float32)
        ids = _want(_require(inputs, 1), np.int32)
        if self.axis != 0 or len(table.shape) != 2:
            raise UnsupportedValue("device Gather supports axis 0 of a 2-D table")
        out = DeviceTensor(ctx, tuple(ids.shape) + (table.shape[1],), np.float32)
        ctx.call("rten_hip_gather_rows_f32", ids.size, table.shape[1], table.shape[0], table.vp, ids.vp, out.vp)
        return [out]


def resolve_axes(nd, axes):
    """resolve_axes (src/ops/mod.rs:259-271): negative axes count from the end, the result is sorted and unique."""
    out = []
    for a in axes:
        if a < -nd or a >= nd:
            raise InvalidValue("Axis is invalid")
        out.append(a + nd if a < 0 else a)
    return sorted(set(out))


SELECT_MAX, SELECT_MIN = 0, 1  # RTEN_HIP_SELECT_*
_DT = {np.dtype(np.float32): 0, np.dtype(np.int32): 1}  # RTEN_HIP_DT_F32 / _I32
REDUCE_L1, REDUCE_SUM_SQUARE, REDUCE_L2, REDUCE_LOG_SUM, REDUCE_LOG_SUM_EXP, REDUCE_PROD = range(6)  # RTEN_HIP_REDUCE_*


def _select_view(x):
    """(view, ABI dtype) of a float32 / int32 operand: a DeviceTensor, or an einsum.View of one (permuted / sliced: reduced in place)."""
    from . import einsum as E
    v = x if isinstance(x, E.View) else E.View(x)
    if v.t.dtype not in _DT:
        raise UnsupportedType
    return v, _DT[v.t.dtype]


def _host_ints(v):
    """A host-side int32 operand (axes, K): numpy array, list or int -> flat list of ints; None stays None."""
    return None if v is None else [int(a) for a in np.asarray(v).reshape(-1)]


def _split_dims(v, axes, *others):
    """The dims of view `v` outside `axes` (kept) and inside (reduced), merged, as the strided reductions' ABI takes them: (kept dims, kept shape, kept
    stride lists, reduced shape, reduced strides).  The first kept stride list is v's own; each of `others`, a full-rank stride list of another view
    of v's shape (TopK's outputs), adds one, and kept dims merge only where every list agrees."""
    from . import einsum as E
    keep = [d for d in range(len(v.shape)) if d not in axes]
    osh, ost = E._merge_axes([v.shape[d] for d in keep], *[[st[d] for d in keep] for st in (v.strides,) + others])
    ish, (ist,) = E._merge_axes([v.shape[d] for d in axes], [v.strides[d] for d in axes])
    if len(osh) > 6 or len(ish) > 6:
        raise UnsupportedValue("more than 6 non-mergeable dims are not supported by the device path")
    return keep, osh, ost, ish, ist


class _ReduceOp(Operator):
    """reduce() (src/ops/reduce.rs:414-520) around one strided kernel: axes attribute or host-side second input, resolved, sorted and de-duplicated; an
    empty slice gives the kernel's value for it.  The slice is read in place through the view's strides.  What the operators do differently, each as
    the reference has it:
      axes_input   a second input replaces the `axes` attribute (not ReduceSum / ReduceMean: their caller resolves it into the attribute)
      int32        the reference also takes Int32Tensor (wrapping arithmetic, or a comparison)
      typed_first  the operand's type is checked before noop_with_empty_axes is looked at (map_value_view! / require_as outside the test,
                   reduce.rs:687,752,827,1215); otherwise only a reduction that runs checks it
      f32_error    falsy: UnsupportedType (map_value_view!); otherwise require_as::<f32>'s cast error
      rank0_copy   a 0-d input returns itself once its axes are validated (reduce.rs:425-428); otherwise it is a slice of one element for the kernel
      _noop        what comes back when noop_with_empty_axes skips the reduction
      _entry       the entry point and its leading arguments"""
    axes_input = True
    int32 = False
    typed_first = True
    f32_error = None
    rank0_copy = False

    def __init__(self, axes=None, keep_dims=True, noop_with_empty_axes=False):
        self.axes, self.keep_dims, self.noop_with_empty_axes = axes, keep_dims, noop_with_empty_axes

    def max_inputs(self):
        return 2

    def _check_type(self, v):
        if v.t.dtype == np.float32 or (self.int32 and v.t.dtype == np.int32):
            return
        if self.f32_error:
            _want(v.t, np.float32)
        raise UnsupportedType

    def _noop(self, ctx, t):
        """`t` is a fresh contiguous copy of the input."""
        return t

    def _reduce(self, ctx, v, axes):
        from . import einsum as E
        keep, osh, (ost,), ish, ist = _split_dims(v, axes)
        y = DeviceTensor(ctx, [v.shape[d] for d in keep], v.t.dtype)
        if y.size:
            ctx.call(*self._entry(), _DT[v.t.dtype], len(osh), E._i64(osh), E._i64(ost), len(ish), E._i64(ish), E._i64(ist), v.t.vp, y.vp)
        return y

    def run(self, ctx, inputs):
        from . import einsum as E
        x = _require(inputs, 0)
        v = x if isinstance(x, E.View) else E.View(x)
        axes = _host_ints(_get(inputs, 1)) if self.axes_input else None
        axes = list(self.axes) if axes is None and self.axes is not None else axes
        if self.typed_first:
            self._check_type(v)
        if not axes and self.noop_with_empty_axes:
            if v.t.dtype.itemsize != 4:
                raise UnsupportedType
            return [self._noop(ctx, E.materialize(ctx, v, dtype=v.t.dtype))]
        self._check_type(v)
        nd = len(v.shape)
        axes = resolve_axes(nd, axes if axes else range(nd))
        if nd == 0 and self.rank0_copy:
            return [E.materialize(ctx, v, dtype=v.t.dtype)]
        y = self._reduce(ctx, v, axes)
        if self.keep_dims:
            y = y.reshape([1 if d in axes else v.shape[d] for d in range(nd)])
        return [y]


class ReduceSum(_ReduceOp):
    """src/ops/reduce.rs:1126-1165 (f32): 16-lane vecmath::Sum order."""
    axes_input, f32_error, rank0_copy = False, True, True
    mean = False

    def _reduce(self, ctx, v, axes):
        from . import einsum as E
        return E.reduce_sum(ctx, v, axes, mean=self.mean)


class ReduceMean(ReduceSum):
    """src/ops/reduce.rs:523-580: vecmath::Sum(slice) / len(slice) as f32 (an empty slice gives NaN)."""
    mean = True


class ReduceMax(_ReduceOp):
    """src/ops/reduce.rs:977-1044 (float32 and int32): a NaN in a slice gives NaN; an empty slice gives the identity (-inf / i32::MIN; ReduceMin:
    +inf / i32::MAX)."""
    int32, rank0_copy = True, True
    op = SELECT_MAX

    def _entry(self):
        return "rten_hip_reduce_minmax_strided", self.op


class ReduceMin(ReduceMax):
    """src/ops/reduce.rs:907-975."""
    op = SELECT_MIN


class _Reduce(_ReduceOp):
    """The six kinds of rten_hip_reduce_strided; a 0-d input is a slice of one element."""
    kind = -1

    def _entry(self):
        return "rten_hip_reduce_strided", self.kind


class ReduceL1(_Reduce):
    """src/ops/reduce.rs:775-845: SumAbs(slice) in the fold_unroll<4> order (float32), wrapping sum of |x| (int32); with the reduction skipped, |x|."""
    kind, int32 = REDUCE_L1, True

    def _noop(self, ctx, t):
        return Abs().run(ctx, [t], in_place=True)[0]


class ReduceSumSquare(_Reduce):
    """src/ops/reduce.rs:1167-1234: SumSquare(slice), fma(x, x, acc) in the fold_unroll<4> order (float32), wrapping sum of x * x (int32); with the
    reduction skipped, x * x (reduce.rs:1216-1218)."""
    kind, int32 = REDUCE_SUM_SQUARE, True

    def _noop(self, ctx, t):
        if t.dtype == np.float32:
            return Mul().run(ctx, [t, t])[0]
        y = DeviceTensor(ctx, t.shape, np.int32)
        if t.size:
            ctx.call("rten_hip_elementwise_nd", L.EW_IMUL, 1, _i64([t.size]), t.vp, L.DT_I32, _i64([1]), t.vp, L.DT_I32, _i64([1]), None, None, y.vp, L.DT_I32)
        return y


class ReduceL2(_Reduce):
    """src/ops/reduce.rs:590-651: sqrt(SumSquare(slice)); float32 only; with the reduction skipped, a copy of the input whatever its type."""
    kind, typed_first = REDUCE_L2, False


class ReduceLogSum(_Reduce):
    """src/ops/reduce.rs:653-708: ln(Sum(slice)), ln = the float64 logarithm rounded once; with the reduction skipped, ln(x)."""
    kind, f32_error = REDUCE_LOG_SUM, True

    def _noop(self, ctx, t):
        return Log().run(ctx, [t], in_place=True)[0]


class ReduceLogSumExp(_Reduce):
    """src/ops/reduce.rs:710-773: m = MaxNum(slice); m when it is not finite, otherwise m + ln(SumExpSub(slice, m)); with the reduction skipped, x."""
    kind, f32_error = REDUCE_LOG_SUM_EXP, True


class ReduceProd(_Reduce):
    """src/ops/reduce.rs:1046-1100: one multiply chain per slice in element order (float32), wrapping product (int32); with the reduction skipped, a
    copy of the input whatever its type."""
    kind, int32, typed_first = REDUCE_PROD, True, False


class LpNormalization(Operator):
    """src/ops/norm.rs:611-693: every lane along `axis` times 1 / norm, norm = SumAbs (p = 1) or sqrt(SumSquare) (p = 2); a zero norm zeroes the lane.
    Defaults as the reference's loader (onnx_registry.rs:1284-1287).  Lanes along a non-last axis are read and written through the axis stride."""

    def __init__(self, axis=-1, p=2):
        self.axis, self.p = axis, p

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        from . import einsum as E
        x = _require(inputs, 0)
        _want(x.t if isinstance(x, E.View) else x, np.float32)
        if self.p not in (1, 2):
            raise UnsupportedValue("`p` must be 1 or 2")
        src = E.materialize(ctx, x) if isinstance(x, E.View) else x  # (the reference normalises a contiguous copy in place)
        nd = len(src.shape)
        ax = _resolve_axis(nd, self.axis)
        y = src if src is not x else DeviceTensor(ctx, src.shape, np.float32)
        v = E.View(src)
        if src.size == 0:
            return [y]
        _, osh, (ost,), _, _ = _split_dims(v, [ax])
        ctx.call("rten_hip_lp_normalize_f32", self.p, len(osh), E._i64(osh), E._i64(ost), v.shape[ax], v.strides[ax], src.vp, y.vp)
        return [y]


class GlobalMaxPool(Operator):
    """src/ops/pooling.rs:549-580: MaxNum over dims 2.. of an input of at least 2 dims, output [N, C, 1, ...]; float32."""

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        from . import einsum as E
        x = _want(_require(inputs, 0), np.float32)
        nd = len(x.shape)
        if nd < 2:
            raise InvalidValue("Input must have at least 2 dims")
        v = E.View(x)
        _, osh, (ost,), ish, ist = _split_dims(v, list(range(2, nd)))
        y = DeviceTensor(ctx, tuple(x.shape[:2]) + (1,) * (nd - 2), np.float32)
        if y.size:
            ctx.call("rten_hip_reduce_minmax_strided", SELECT_MAX, _DT[x.dtype], len(osh), E._i64(osh), E._i64(ost), len(ish), E._i64(ish), E._i64(ist), x.vp, y.vp)
        return [y]


class ArgMax(Operator):
    """src/ops/reduce.rs:64-160: int32 index along `axis` following Iterator::max_by with cmp_nan_greater -- the FIRST NaN if the lane holds
    one, otherwise the LAST element equal to the extreme.  select_last_index != 0 is refused as by the reference's loader (onnx_registry.rs:769)."""
    op = SELECT_MAX

    def __init__(self, axis=0, keep_dims=True, select_last_index=0):
        if select_last_index:
            raise UnsupportedValue("select_last_index is not supported")
        self.axis, self.keep_dims = axis, keep_dims

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        from . import einsum as E
        v, dt = _select_view(_require(inputs, 0))
        nd = len(v.shape)
        ax = _resolve_axis(nd, self.axis)
        if v.shape[ax] == 0:
            raise InvalidValue("Cannot select index from empty sequence")
        keep, osh, (ost,), _, _ = _split_dims(v, [ax])
        y = DeviceTensor(ctx, [v.shape[d] for d in keep], np.int32)
        if y.size:
            ctx.call("rten_hip_arg_minmax_strided", self.op, dt, len(osh), E._i64(osh), E._i64(ost), v.shape[ax], v.strides[ax], v.t.vp, y.vp)
        if self.keep_dims:
            y = y.reshape([1 if d == ax else v.shape[d] for d in range(nd)])
        return [y]


class ArgMin(ArgMax):
    """src/ops/reduce.rs:162-215."""
    op = SELECT_MIN


class TopK(Operator):
    """src/ops/reduce.rs:1236-1356: inputs X, K (host-side int32 scalar or 1-element vector); outputs values (X's type) and int32 indices.  NaN is
    greater than every number whatever `largest` says; equal values by ascending index.  The result is always sorted (with sorted == 0 the reference
    leaves an unspecified order of the same pairs)."""

    def __init__(self, axis=-1, largest=True, sorted=True):
        self.axis, self.largest, self.sorted = axis, largest, sorted

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        from . import einsum as E
        v, dt = _select_view(_require(inputs, 0))
        kv = _host_ints(_require(inputs, 1))
        if len(kv) != 1:
            raise InvalidValue("Expected scalar value")
        k = kv[0]
        if k < 0:
            raise InvalidValue("k must be positive")
        nd = len(v.shape)
        ax = _resolve_axis(nd, -1 if self.axis is None else self.axis)
        out_shape = [k if d == ax else v.shape[d] for d in range(nd)]
        values, indices = DeviceTensor(ctx, out_shape, v.t.dtype), DeviceTensor(ctx, out_shape, np.int32)
        if k == 0:
            return [values, indices]
        if k > v.shape[ax]:
            raise InvalidValue("k > dimension size")
        if values.size:
            ov = E.View(values)
            _, osh, (ost, oost), _, _ = _split_dims(v, [ax], ov.strides)
            try:
                ctx.call("rten_hip_topk_strided", 1 if self.largest else 0, dt, len(osh), E._i64(osh), E._i64(ost), E._i64(oost), v.shape[ax], v.strides[ax],
                         k, v.t.vp, values.vp, indices.vp, ov.strides[ax])
            except L.HipError as e:
                if e.code == L.ERR_UNSUPPORTED:
                    raise UnsupportedValue(e.msg)
                raise
        return [values, indices]


class Einsum(Operator):
    """src/ops/einsum.rs:21-108: any number of f32 inputs, `equation` attribute.  The planner and the strided lowering
    are in rten_amd/einsum.py."""

    def __init__(self, equation: str):
        self.equation = equation

    def max_inputs(self):
        return None

    def run(self, ctx, inputs):
        from . import einsum as E
        xs = [_want(_require(inputs, i), np.float32) for i in range(len(inputs))]
        return [E.einsum(ctx, xs, self.equation)]


# ------------------------------------------------------------------------------------------ Resize / Upsample / Split
RESIZE_MODES = {"nearest": L.RESIZE_MODE_NEAREST, "linear": L.RESIZE_MODE_LINEAR}
RESIZE_COORDS = {"half_pixel": L.RESIZE_COORD_HALF_PIXEL, "asymmetric": L.RESIZE_COORD_ASYMMETRIC, "align_corners": L.RESIZE_COORD_ALIGN_CORNERS,
                 "pytorch_half_pixel": L.RESIZE_COORD_PYTORCH_HALF_PIXEL}
RESIZE_NEAREST = {"round_prefer_floor": L.RESIZE_NEAREST_ROUND_PREFER_FLOOR, "round_prefer_ceil": L.RESIZE_NEAREST_ROUND_PREFER_CEIL,
                  "floor": L.RESIZE_NEAREST_FLOOR, "ceil": L.RESIZE_NEAREST_CEIL}


def _host_values(t):
    """A scales / sizes / split operand: a numpy array or list as given, a DeviceTensor read back."""
    return t.numpy() if isinstance(t, DeviceTensor) else np.asarray(t)


def _optional_operand(t, dtype, what):
    """get_optional_input (src/ops/resize.rs:496-507): an absent or empty tensor is missing; otherwise a 1-D operand."""
    if t is None:
        return None
    a = _host_values(t)
    if a.size == 0:
        return None
    if a.ndim != 1:
        raise InvalidValue(f"{what} must have 1 dims")
    return a.astype(dtype)


def resize_geometry(in_shape, scales=None, sizes=None):
    """calc_output_size (src/ops/resize.rs:273-308): (output sizes, f32 inverse scales).  size = floor(in * scale) in f32 (`as i32` saturates,
    NaN -> 0) with inv_scale = 1 / scale, or the given size with in / size."""
    target = scales if scales is not None else sizes
    if len(target) != len(in_shape):
        raise IncompatibleInputShapes("scales/sizes length should equal input rank")
    out, inv = [], []
    with np.errstate(all="ignore"):
        for d, n in enumerate(in_shape):
            if scales is not None:
                s = np.float32(scales[d])
                f = np.floor(np.float32(n) * s)
                out.append(0 if np.isnan(f) else int(max(min(f, 2 ** 31 - 1), -(2 ** 31))))
                inv.append(np.float32(1) / s)
            else:
                o = int(np.int32(sizes[d]))
                out.append(o)
                inv.append(np.float32(n) / np.float32(o))
    if any(v < 0 for v in out):
        raise InvalidValue("scales/sizes must be positive")
    return out, inv


def _resize_planes(in_shape, out, inv):
    """resize_impl (src/ops/resize.rs:334-408): the [planes, H, W] view (planes, in_h, in_w, out_h, out_w, inv_y, inv_x); an axis the input is
    expanded along has scale 1."""
    s, o, one = tuple(in_shape), tuple(out), np.float32(1)
    if len(s) == 4 and s[:2] == o[:2]:
        return s[0] * s[1], s[2], s[3], o[2], o[3], inv[2], inv[3]
    if len(s) == 3 and s[:2] == o[:2]:  # NCW, tried before NHW
        return s[0] * s[1], 1, s[2], 1, o[2], one, inv[2]
    if len(s) == 3 and s[0] == o[0]:  # NHW
        return s[0], s[1], s[2], o[1], o[2], inv[1], inv[2]
    if len(s) == 2:
        return 1, s[0], s[1], o[0], o[1], inv[0], inv[1]
    if len(s) == 1:
        return 1, 1, s[0], 1, o[0], one, inv[0]
    raise UnsupportedValue("Only 1D to 4D inputs are supported with up to two resized dimensions")


def _enum(v, table):
    return table[v] if isinstance(v, str) else int(v)


class Resize(Operator):
    """src/ops/resize.rs:470-606 (rten_hip_resize_f32): inputs X (f32), roi (read by tf_crop_and_resize only, which is unsupported), scales (f32) or
    sizes (i32); an absent or empty scales / sizes is missing.  An output of the input's shape is a copy, whatever the scales."""

    def __init__(self, mode="nearest", coord_mode="half_pixel", nearest_mode="round_prefer_floor"):
        self.mode, self.coord_mode, self.nearest_mode = mode, coord_mode, nearest_mode

    def max_inputs(self):
        return 4

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        scales = _optional_operand(_get(inputs, 2), np.float32, "scales")
        sizes = _optional_operand(_get(inputs, 3), np.int32, "sizes")
        if scales is None and sizes is None:
            raise MissingInputs
        return [self.resize(ctx, x, scales=scales, sizes=None if scales is not None else sizes)]

    def resize(self, ctx, x, scales=None, sizes=None):
        x = _want(x, np.float32)
        out, inv = resize_geometry(x.shape, scales, sizes)
        if tuple(out) == tuple(x.shape):  # nothing resized (resize.rs:352)
            y = DeviceTensor(ctx, out, np.float32)
            if x.size:
                ctx.call("rten_hip_memcpy_d2d", y.vp, x.vp, C.c_size_t(4 * x.size))
            return y
        planes, ih, iw, oh, ow, sy, sx = _resize_planes(x.shape, out, inv)
        y = DeviceTensor(ctx, out, np.float32)
        if y.size:
            ctx.call("rten_hip_resize_f32", _enum(self.mode, RESIZE_MODES), _enum(self.coord_mode, RESIZE_COORDS), _enum(self.nearest_mode, RESIZE_NEAREST),
                     planes, ih, iw, oh, ow, float(sy), float(sx), x.vp, y.vp)
        return y


class Upsample(Resize):
    """src/ops/resize.rs:610-652: the deprecated form of Resize -- scales (input 1) required, asymmetric coordinates, floor."""

    def __init__(self, mode="nearest"):
        super().__init__(mode, "asymmetric", "floor")

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        scales = _host_values(_require(inputs, 1))
        if scales.ndim != 1:
            raise InvalidValue("scales must have 1 dims")
        return [self.resize(ctx, x, scales=scales.astype(np.float32))]


class GridSample(Operator):
    """src/ops/grid_sample.rs:17-145 (rten_hip_grid_sample_f32): bilinear sampling with zero padding of X [N, C, H, W] at grid [N, H_out, W_out, 2].
    The loaders refuse every other mode / padding_mode (onnx_registry.rs:1203-1212)."""

    def __init__(self, align_corners=False):
        self.align_corners = align_corners

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        if len(x.shape) != 4:
            raise InvalidValue("input must have 4 dims (NCHW)")
        grid = _want(_require(inputs, 1), np.float32)
        if len(grid.shape) != 4:
            raise InvalidValue("grid must have 4 dims")
        if grid.shape[0] != x.shape[0]:
            raise IncompatibleInputShapes("Batch size of input and grid must match")
        if grid.shape[3] != 2:
            raise UnsupportedValue("Unsupported grid coordinate size")
        n, c, h, w = x.shape
        y = DeviceTensor(ctx, (n, c, grid.shape[1], grid.shape[2]), np.float32)
        if y.size:
            ctx.call("rten_hip_grid_sample_f32", 1 if self.align_corners else 0, n, c, h, w, grid.shape[1], grid.shape[2], x.vp, grid.vp, y.vp)
        return [y]


DEPTH_TO_SPACE_PERMS = {"DCR": (0, 3, 4, 1, 5, 2), "CRD": (0, 1, 4, 2, 5, 3)}


class DepthToSpace(Operator):
    """src/ops/layout.rs:22-103: ONE rten_hip_transpose_b32 launch on the 6-D view the reference builds -- DCR [n, b, b, c', h, w] by (0, 3, 4, 1, 5, 2),
    CRD [n, c', b, b, h, w] by (0, 1, 4, 2, 5, 3) -- read as [n, c', h * b, w * b].  float32 only, as the reference's run()."""

    def __init__(self, block_size, mode="DCR"):
        if mode not in DEPTH_TO_SPACE_PERMS:  # (the reference's DepthToSpaceMode has the two variants only; its loader refuses any other string)
            raise UnsupportedValue("DepthToSpace mode must be DCR or CRD")
        self.block_size, self.mode = block_size, mode

    def max_inputs(self):
        return 1

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        if self.mode not in DEPTH_TO_SPACE_PERMS:
            raise UnsupportedValue("DepthToSpace mode must be DCR or CRD")
        b = int(self.block_size)
        if b <= 0:
            raise InvalidValue("`block_size` must be > 0")
        if len(x.shape) != 4:
            raise InvalidValue("input must have 4 dims (NCHW)")
        n, c, h, w = x.shape
        if c % (b * b) != 0:
            raise InvalidValue("input channels must be a multiple of `block_size` squared")
        nc = c // (b * b)
        view = (n, b, b, nc, h, w) if self.mode == "DCR" else (n, nc, b, b, h, w)
        y = DeviceTensor(ctx, (n, nc, h * b, w * b), np.float32)
        if y.size:
            ctx.call("rten_hip_transpose_b32", 6, (C.c_int64 * 6)(*view), (C.c_int32 * 6)(*DEPTH_TO_SPACE_PERMS[self.mode]), x.vp, y.vp)
        return [y]


def _scalar_i32(t):
    """The reference's `require_as::<i32>`: an int32 operand of one element, of any rank (a numpy array / int as given, a DeviceTensor read back)."""
    a = _host_values(t)
    if a.dtype.kind not in "iu":
        raise OpError("InputCastFailed", "expected int32 tensor")
    if a.size != 1:
        raise OpError("InputCastFailed", "expected tensor with 0 dims")
    return int(a.reshape(()))


def _b32_numeric(x):
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.int32)):
        raise UnsupportedType
    return x


class CumSum(Operator):
    """src/ops/reduce.rs:217-297 (rten_hip_cumsum_b32): inputs (data, axis); float32 / int32.  Per lane along the axis acc = 0; prev = acc; acc += x;
    y = exclusive ? prev : acc, from the end if `reverse` -- the f32 sum strictly sequential, int32 wrapping.  The axis is a host-side operand.  A lane with
    inner == 1 takes the kernel's row form, any other the column form (the entry point chooses)."""

    def __init__(self, exclusive=False, reverse=False):
        self.exclusive, self.reverse = exclusive, reverse

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _b32_numeric(_require(inputs, 0))
        axis = _scalar_i32(_require(inputs, 1))
        ax = _resolve_axis(len(x.shape), axis)
        outer = int(np.prod(x.shape[:ax], dtype=np.int64))
        inner = int(np.prod(x.shape[ax + 1:], dtype=np.int64))
        y = DeviceTensor(ctx, x.shape, x.dtype)
        if y.size:
            ctx.call("rten_hip_cumsum_b32", _DT[x.dtype], 1 if self.exclusive else 0, 1 if self.reverse else 0, outer, x.shape[ax], inner, x.vp, y.vp)
        return [y]

    def batch_coupled(self, x_shape, axis):
        """Sub-batch chains split dim 0: the rows are coupled when the sum runs along it."""
        return _resolve_axis(len(x_shape), axis) == 0


class GatherElements(Operator):
    """src/ops/gather.rs:196-319 (rten_hip_gather_elements_b32): y[i0, ..] = x[i0, .., indices[i0, ..], ..] along `axis` on the input trimmed to the
    indices' extent; 4-byte data, int32 indices, at most 6 dims.  Negative indices add the axis length once.  Out-of-range indices: host-side
    indices (a numpy array) are refused with the reference's message; device indices are CLAMPED by the kernel -- the same deliberate deviation as
    Gather's rten_hip_gather_axis_b32, because nothing is read back."""

    def __init__(self, axis=0):
        self.axis = axis

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        ids = _require(inputs, 1)
        host_ids = None
        if not isinstance(ids, DeviceTensor):
            host_ids = np.asarray(ids)
            if host_ids.dtype != np.dtype(np.int32):
                raise OpError("InputCastFailed", "expected int32 tensor")
        else:
            _want(ids, np.int32)
        if x.dtype.itemsize != 4:
            raise UnsupportedType
        ishape = tuple(host_ids.shape) if host_ids is not None else tuple(ids.shape)
        if len(ishape) != len(x.shape):
            raise IncompatibleInputShapes("Input and indices must have same rank")
        ax = _resolve_axis(len(x.shape), self.axis)
        if any(d != ax and ishape[d] > x.shape[d] for d in range(len(ishape))):
            raise IncompatibleInputShapes("`indices` size must be <= input size in non-axis dimensions")
        if len(x.shape) > 6:
            raise UnsupportedValue("GatherElements supports at most 6 dims")
        n = int(np.prod(ishape, dtype=np.int64))
        alen = x.shape[ax]
        if n and alen == 0:
            raise InvalidValue("Entry in `indices` is out of range")
        if host_ids is not None:
            if n and (host_ids.min() < -alen or host_ids.max() >= alen):
                raise InvalidValue("Entry in `indices` is out of range")
            ids = DeviceTensor.from_numpy(ctx, host_ids)
        y = DeviceTensor(ctx, ishape, x.dtype)
        if y.size:
            ctx.call("rten_hip_gather_elements_b32", len(x.shape), _i64(x.shape), _i64(ishape), ax, x.vp, ids.vp, y.vp)
        return [y]

    def batch_coupled(self, x_shape):
        return _resolve_axis(len(x_shape), self.axis) == 0


class Trilu(Operator):
    """src/ops/trilu.rs:15-97 (rten_hip_trilu_b32): inputs (data, k); k optional (0), a host-side operand.  Per inner matrix delta = row + k - col, kept when
    delta <= 0 (upper) / delta >= 0 (lower), else the all-zero word."""

    def __init__(self, upper=True):
        self.upper = upper

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _b32_numeric(_require(inputs, 0))
        k_t = _get(inputs, 1)
        k = 0 if k_t is None else _scalar_i32(k_t)
        if len(x.shape) < 2:
            raise InvalidValue("Input must have >= 2 dims")
        y = DeviceTensor(ctx, x.shape, x.dtype)
        if y.size:
            ctx.call("rten_hip_trilu_b32", 1 if self.upper else 0, k, int(np.prod(x.shape[:-2], dtype=np.int64)), x.shape[-2], x.shape[-1], x.vp, y.vp)
        return [y]

    def batch_coupled(self, x_shape):
        """On a rank-2 operand dim 0 is the matrix row."""
        return len(x_shape) == 2


class Tile(Operator):
    """src/ops/concat.rs:239-300 (rten_hip_tile_b32): inputs (data, repeats); y.shape[d] = x.shape[d] * repeats[d], y[i] = x[i mod x.shape].  `repeats` is a
    host-side 1-D operand; a length other than the rank, or a negative entry, is "invalid repeats"."""

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        x = _b32_numeric(_require(inputs, 0))
        r = _host_values(_require(inputs, 1))
        if r.dtype.kind not in "iu":
            raise OpError("InputCastFailed", "expected int32 tensor")
        if r.ndim != 1:
            raise OpError("InputCastFailed", "expected tensor with 1 dims")
        repeats = [int(v) for v in r]
        if len(repeats) != len(x.shape) or any(v < 0 for v in repeats):
            raise InvalidValue("invalid repeats")
        if len(x.shape) > 6:
            raise UnsupportedValue("Tile supports at most 6 dims")
        y = DeviceTensor(ctx, [s * v for s, v in zip(x.shape, repeats)], x.dtype)
        if y.size:
            ctx.call("rten_hip_tile_b32", len(x.shape), _i64(x.shape), _i64(repeats), x.vp, y.vp)
        return [y]

    @staticmethod
    def batch_coupled(repeats):
        return len(repeats) > 0 and int(repeats[0]) != 1


class Split(Operator):
    """src/ops/split.rs:34-136 on 4-byte tensors (one rten_hip_copy_strided_b32 per piece): the sizes of input 1, else `num_outputs`, else the
    node's output count as equal chunks of ceil(dim / n) -- the last piece is smaller, and there may be fewer than n pieces (5 split 4 ways
    gives 3)."""

    def __init__(self, axis=0, num_outputs=None, node_outputs=1):
        self.axis, self.num_outputs, self.node_outputs = axis, num_outputs, node_outputs

    def max_inputs(self):
        return 2

    def pieces(self, dim, sizes=None):
        """(start, length) along the axis of every piece."""
        if sizes is not None:
            sizes = [int(s) for s in sizes]
            if any(s < 0 for s in sizes):
                raise InvalidValue("Split sizes must be >= 0")
            if sum(sizes) != dim:
                raise InvalidValue("Split sizes do not sum to dimension size")
            return [(sum(sizes[:k]), s) for k, s in enumerate(sizes)]
        n = self.node_outputs if self.num_outputs is None else self.num_outputs
        if n == 0:
            raise InvalidValue("num_outputs must be > 0")
        if n > dim:
            raise InvalidValue("num_outputs exceeds dim size")
        chunk = -(-dim // n)
        return [(a, min(chunk, dim - a)) for a in range(0, dim, chunk)]

    def run(self, ctx, inputs):
        x = _require(inputs, 0)
        nd = len(x.shape)
        ax = _resolve_axis(nd, self.axis)
        s = _get(inputs, 1)
        pieces = self.pieces(x.shape[ax], None if s is None else _host_values(s).reshape(-1))
        if x.dtype.itemsize != 4:
            raise UnsupportedType
        if nd > 6:
            raise UnsupportedValue("Split: more than 6 dims on the device path")
        strides = [int(np.prod(x.shape[d + 1:], dtype=np.int64)) for d in range(nd)]
        outs = []
        for start, length in pieces:
            shape = list(x.shape)
            shape[ax] = length
            y = DeviceTensor(ctx, shape, x.dtype)
            if y.size:
                ctx.call("rten_hip_copy_strided_b32", nd, (C.c_int64 * nd)(*shape), (C.c_int64 * nd)(*strides), C.c_void_p(x.ptr + 4 * start * strides[ax]), y.vp)
            outs.append(y)
        return outs


def _nms_scalar(t, index, kind, what):
    """get_as::<i32 / f32> (src/operator.rs:790-806) of one of NonMaxSuppression's optional operands: absent -> None; a host value (numpy array or
    Python number) of one element, of any rank.  A device tensor is refused: the graph executor hands constants and shape arithmetic over as host values."""
    if t is None:
        return None
    if isinstance(t, DeviceTensor):
        raise UnsupportedValue(f"NonMaxSuppression: {what} (input {index}) must be a host value, a constant or shape arithmetic; it is device data")
    a = np.asarray(t)
    if a.dtype.kind not in kind:
        raise OpError("InputCastFailed", "expected int32 tensor" if kind == "iu" else "expected float32 tensor")
    if a.size != 1:
        raise OpError("InputCastFailed", "expected tensor with 0 dims")
    return a.reshape(())


class NonMaxSuppression(Operator):
    """src/ops/non_max_suppression.rs:40-233 (rten_hip_non_max_suppression_f32): inputs boxes [N, B, 4], scores [N, C, B] and, optional and host-side,
    max_output_boxes_per_class (int; ABSENT means no limit, the reference's default, and an int64 is narrowed with saturation as the loader does),
    iou_threshold and score_threshold (float32, default 0).  The reference's rule, not textbook NMS (the entry point's comment in include/rten_hip.h states
    it): one selected list across images and classes, candidates in (n, b) order, hull IoU, removals by a rejected candidate stay.  The result is an int32
    [count, 3] tensor of [n, class, b] rows: its shape depends on device values, so the call synchronises once and cannot be captured."""

    def __init__(self, center_point_box=0):
        self.center_point_box = center_point_box

    def max_inputs(self):
        return 5

    def run(self, ctx, inputs):
        if len(inputs) > 5:
            raise InvalidValue("NonMaxSuppression takes at most 5 inputs")
        boxes, scores = _want(_require(inputs, 0), np.float32), _want(_require(inputs, 1), np.float32)
        for t in (boxes, scores):
            if len(t.shape) != 3:
                raise OpError("InputCastFailed", "expected tensor with 3 dims")
        cap = _nms_scalar(_get(inputs, 2), 2, "iu", "max_output_boxes_per_class")
        iou = _nms_scalar(_get(inputs, 3), 3, "f", "iou_threshold")
        score = _nms_scalar(_get(inputs, 4), 4, "f", "score_threshold")
        if self.center_point_box not in (0, 1):
            raise InvalidValue("center_point_box must be 0 or 1")
        n, b, coords = boxes.shape
        sn, c, sb = scores.shape
        if coords != 4:
            raise InvalidValue("`boxes` last dimension should have size 4")
        if n != sn or b != sb:
            raise IncompatibleInputShapes("`boxes` and `scores` have incompatible shapes")
        if c == 0 or n * b == 0:
            return [DeviceTensor(ctx, (0, 3), np.int32)]
        rows = DeviceTensor(ctx, (n * b, 3), np.int32)
        count = C.c_int64(0)
        cap_v = 0 if cap is None else max(-2 ** 31, min(2 ** 31 - 1, int(cap)))  # saturating_cast_i64_to_i32
        ctx.call("rten_hip_non_max_suppression_f32", int(self.center_point_box), n, c, b, boxes.vp, scores.vp, 0 if cap is None else 1, cap_v,
                 C.c_float(0.0 if iou is None else float(np.float32(iou))), C.c_float(0.0 if score is None else float(np.float32(score))), rows.vp, C.byref(count))
        return [rows.view((int(count.value), 3))]

    def batch_coupled(self):
        """One selected list serves every image: sub-batch chains would give other rows."""
        return True


def _fft_host_int(t, index, op, what):
    """get_as::<i32> of a DFT / STFT size operand: absent -> None; a host value (numpy array or Python int) of one element, of any rank.  A device tensor
    is refused, worded like Pad's: the graph executor hands constants and shape arithmetic over as host values."""
    if t is None:
        return None
    if isinstance(t, DeviceTensor):
        raise UnsupportedValue(f"{op}: {what} (input {index}) must be a constant or computable from the input shapes (it depends on device data)")
    a = np.asarray(t)
    if a.dtype.kind not in "iu":
        raise OpError("InputCastFailed", "expected int32 tensor")
    if a.size != 1:
        raise OpError("InputCastFailed", "expected tensor with 0 dims")
    return int(a.reshape(()))


def _fft_limit(op, what, n):
    if n > L.FFT_MAX:
        raise UnsupportedValue(f"{op} {what} of length {n} exceeds the limit of {L.FFT_MAX} points (RTEN_HIP_FFT_MAX)")


class DFT(Operator):
    """src/ops/fft.rs:200-373 (rten_hip_dft_f32): inputs (x [..., n, 1 | 2], dft_length?, axis?), float32; dft_length and axis are host-side operands
    (axis default -2, the opset-20 form; an opset < 20 node's `axis` attribute arrives as that input).  The lane is truncated or zero-filled to n_fft =
    dft_length, else the axis length, else 2 * (len - 1) for IRFFT (inverse and onesided: complex half spectrum in, real signal out).  onesided forward
    (real input only) keeps n_fft / 2 + 1 bins; the inverse scales by 1.0f / n_fft.  An axis other than ndim - 2 is moved there and back with
    rten_hip_transpose_b32, as the reference permutes.  Lengths above RTEN_HIP_FFT_MAX are UnsupportedValue.  The contract is an error bound against the
    exact transform (include/rten_hip.h), not bit-identity with the reference's FFT library."""

    def __init__(self, inverse=False, onesided=False):
        self.inverse, self.onesided = bool(inverse), bool(onesided)

    def max_inputs(self):
        return 3

    def run(self, ctx, inputs):
        x = _want(_require(inputs, 0), np.float32)
        dft_length = _fft_host_int(_get(inputs, 1), 1, "DFT", "dft_length")
        axis = _fft_host_int(_get(inputs, 2), 2, "DFT", "axis")
        axis = -2 if axis is None else axis
        nd = len(x.shape)
        if nd < 2:
            raise InvalidValue("DFT input must have at least 2 dims")
        comp = x.shape[-1]
        if comp not in (1, 2):
            raise InvalidValue("Last dimension of DFT input must have size 1 or 2")
        irfft = self.inverse and self.onesided
        if irfft and comp != 2:
            raise InvalidValue("Inverse one-sided DFT (IRFFT) requires complex input")
        if self.onesided and not self.inverse and comp == 2:
            raise InvalidValue("DFT cannot be one-sided if input is complex")
        ax = _resolve_axis(nd, axis)
        if ax == nd - 1:
            raise InvalidValue("DFT axis cannot be the complex dimension")
        n_in = x.shape[ax]
        if dft_length is not None:
            if dft_length < 1:
                raise InvalidValue("dft_length must be >= 1")
            n_fft = dft_length
        else:
            n_fft = 2 * max(n_in - 1, 0) if irfft else n_in
        _fft_limit("DFT", "transform", n_fft)
        out_len = n_fft // 2 + 1 if self.onesided and not self.inverse else n_fft
        out_comp = 1 if irfft else 2
        fwd = [d for d in range(nd) if d not in (ax, nd - 1)] + [ax, nd - 1]
        tshape = [x.shape[d] for d in fwd]
        lanes = int(np.prod(tshape[:-2], dtype=np.int64))
        oshape_t = tshape[:-2] + [out_len, out_comp]
        flags = (1 if self.inverse else 0, 1 if self.onesided else 0)
        if ax == nd - 2:
            y = DeviceTensor(ctx, oshape_t, np.float32)
            if y.size:
                ctx.call("rten_hip_dft_f32", lanes, n_in, n_fft, comp, *flags, x.vp, y.vp)
            return [y]
        if nd > 6:
            raise UnsupportedValue("DFT along an axis other than ndim - 2 of more than 6 dims is not supported by the device path")
        back = [fwd.index(d) for d in range(nd)]
        y = DeviceTensor(ctx, [oshape_t[back[d]] for d in range(nd)], np.float32)
        if y.size:
            i64 = lambda v: (C.c_int64 * len(v))(*v)
            i32 = lambda v: (C.c_int32 * len(v))(*v)
            t, u = DeviceTensor(ctx, tshape, np.float32), DeviceTensor(ctx, oshape_t, np.float32)
            if x.size:
                ctx.call("rten_hip_transpose_b32", nd, i64(list(x.shape)), i32(fwd), x.vp, t.vp)
            ctx.call("rten_hip_dft_f32", lanes, n_in, n_fft, comp, *flags, t.vp, u.vp)
            ctx.call("rten_hip_transpose_b32", nd, i64(oshape_t), i32(back), u.vp, y.vp)
        return [y]

    def batch_coupled(self, x_shape, axis=-2):
        """Sub-batch chains split dim 0: the rows are coupled when the transform runs along it."""
        return _resolve_axis(len(x_shape), axis) == 0


class STFT(Operator):
    """src/ops/fft.rs:22-133 (rten_hip_stft_f32): inputs (signal [batch, len] or [batch, len, 1 | 2], frame_step, window?, frame_length?), float32;
    frame_step and frame_length are host-side operands, the window a device tensor or a host array (uploaded).  n_fft is frame_length, else the window's
    length; frame f is signal[f * frame_step + k] * window[k], read straight from the signal; the output is [batch, n_frames, bins, 2], n_frames =
    (len - n_fft) / frame_step + 1, bins = n_fft / 2 + 1 when onesided (real signal only).  Frames above RTEN_HIP_FFT_MAX are UnsupportedValue."""

    def __init__(self, onesided=True):
        self.onesided = bool(onesided)

    def max_inputs(self):
        return 4

    def run(self, ctx, inputs):
        signal = _want(_require(inputs, 0), np.float32)
        frame_step = _fft_host_int(_require(inputs, 1), 1, "STFT", "frame_step")
        window = _get(inputs, 2)
        frame_length = _fft_host_int(_get(inputs, 3), 3, "STFT", "frame_length")
        if window is not None:
            if not isinstance(window, DeviceTensor):
                w = np.asarray(window)
                if w.dtype != np.dtype(np.float32):
                    raise OpError("InputCastFailed", "expected float32 tensor")
                window = DeviceTensor.from_numpy(ctx, w)
            _want(window, np.float32)
            if len(window.shape) != 1:
                raise OpError("InputCastFailed", "expected tensor with 1 dims")
        if len(signal.shape) == 2:
            batch, signal_len = signal.shape
            comp = 1
        elif len(signal.shape) == 3:
            batch, signal_len, comp = signal.shape
        else:
            raise InvalidValue("signal must have 2 or 3 dims")
        if frame_length is not None and not 1 <= frame_length <= signal_len:
            raise InvalidValue("frame_length must be in range [1, signal_length]")
        if frame_step <= 0:
            raise InvalidValue("frame_step must be > 0")
        if frame_length is not None and window is not None and frame_length != window.shape[0]:
            raise InvalidValue("window length must equal frame_length")
        n_fft = frame_length if frame_length is not None else (window.shape[0] if window is not None else None)
        if n_fft is None:
            raise InvalidValue("Either frame_length or window must be set")
        if comp not in (1, 2):
            raise InvalidValue("Last dimension of signal must have size 1 or 2")
        if comp == 2 and self.onesided:
            raise InvalidValue("FFT cannot be one-sided if input is complex")
        if not 1 <= n_fft <= signal_len:  # (a window that is empty or longer than the signal: the reference's frame count is meaningless there)
            raise InvalidValue("frame_length must be in range [1, signal_length]")
        _fft_limit("STFT", "frame", n_fft)
        n_frames = (signal_len - n_fft) // frame_step + 1
        bins = n_fft // 2 + 1 if self.onesided else n_fft
        y = DeviceTensor(ctx, (batch, n_frames, bins, 2), np.float32)
        if y.size:
            ctx.call("rten_hip_stft_f32", batch, signal_len, comp, frame_step, n_fft, 1 if self.onesided else 0, _vp(window), signal.vp, y.vp)
        return [y]


RNN_DIRECTIONS = {"forward":L.RNN_FORWARD, "reverse": L.RNN_REVERSE, "bidirectional": L.RNN_BIDIRECTIONAL}


def _rnn_dims(t, ndim, what, names=None):
    """static_dims! (src/operator.rs:210-241): "<name> must have N dims (<names>)"."""
    if len(t.shape) != ndim:
        raise InvalidValue(f"{what} must have {ndim} dims" + (f" ({names})" if names else ""))
    return _want(t, np.float32)


class _Recurrent(Operator):
    """What GRU and LSTM share (src/ops/rnn.rs): the direction attribute, output allocation and the C-ABI call.  `outputs` selects which of
    Y, Y_h (, Y_c) are computed: an entry that is False comes back as None (a graph node may leave outputs unnamed)."""

    GATES = 0

    def _direction(self):
        if self.direction not in RNN_DIRECTIONS:
            raise InvalidValue(f"unknown direction {self.direction!r}")
        return RNN_DIRECTIONS[self.direction]

    def _launch(self, ctx, symbol, x, operands, n_out, outputs):
        seq, batch, n_in = x.shape
        dirs = 2 if self.direction == "bidirectional" else 1
        hidden = operands[0].shape[1] // self.GATES
        want = list(outputs) if outputs is not None else [True] * n_out
        shapes = [(seq, dirs, batch, hidden)] + [(dirs, batch, hidden)] * (n_out - 1)
        outs = [DeviceTensor(ctx, sh, np.float32) if w else None for sh, w in zip(shapes, want)]
        geometry = [seq, batch, n_in, hidden, self._direction()] + ([1] if self.GATES == 3 else []) + [0, 0]  # (GRU: linear_before_reset; X contiguous)
        try:
            ctx.call(symbol, *geometry, x.vp, *[_vp(t) for t in operands], *[_vp(t) for t in outs])
        except L.HipError as e:
            if e.code == L.ERR_UNSUPPORTED:
                raise UnsupportedValue(e.msg)
            raise
        return outs


class GRU(_Recurrent):
    """src/ops/rnn.rs:107-383.  Inputs X [seq, batch, input], W [dirs, 3 * hidden, input], R [dirs, 3 * hidden, hidden], B [dirs, 6 * hidden]
    (optional), sequence_lens (ignored, as in the reference), initial_h [dirs, batch, hidden] (optional); gate order update, reset, hidden.
    Outputs Y [seq, dirs, batch, hidden] and Y_h [dirs, batch, hidden]."""

    GATES = 3

    def __init__(self, direction="forward", hidden_size=0, linear_before_reset=False):
        self.direction, self.hidden_size, self.linear_before_reset = direction, hidden_size, linear_before_reset

    def max_inputs(self):
        return 6

    def run(self, ctx, inputs, outputs=None):
        if not self.linear_before_reset:
            raise UnsupportedValue("`linear_before_reset=0` is not supported")
        x = _rnn_dims(_require(inputs, 0), 3, "input", "seq, batch, input")
        w = _rnn_dims(_require(inputs, 1), 3, "weights", "dir, hidden x 3, input")
        r = _rnn_dims(_require(inputs, 2), 3, "recurrent_weights")
        b, h0 = _get(inputs, 3), _get(inputs, 5)
        if b is not None:
            _rnn_dims(b, 2, "bias", "dir, hidden x 6")
        if h0 is not None:
            _rnn_dims(h0, 3, "initial_hidden")
        return self._launch(ctx, "rten_hip_gru_f32", x, [w, r, b, h0], 2, outputs)


class LSTM(_Recurrent):
    """src/ops/rnn.rs:385-660.  Inputs X, W [dirs, 4 * hidden, input], R [dirs, 4 * hidden, hidden], B [dirs, 8 * hidden] (optional), sequence_lens
    (ignored), initial_h, initial_c [dirs, batch, hidden] (optional); gate order input, output, forget, cell.  Outputs Y, Y_h, Y_c.  tanh(c) in
    h = o * tanh(c) is the vecmath tanh (the reference calls the host's libm there: docs/KERNELS.md)."""

    GATES = 4

    def __init__(self, direction="forward", hidden_size=0):
        self.direction, self.hidden_size = direction, hidden_size

    def max_inputs(self):
        return 7

    def run(self, ctx, inputs, outputs=None):
        x = _rnn_dims(_require(inputs, 0), 3, "input", "seq, batch, input")
        w = _rnn_dims(_require(inputs, 1), 3, "weights", "dir, hidden x 4, input")
        r = _rnn_dims(_require(inputs, 2), 3, "recurrent_weights", "dir, hidden x 4, hidden")
        if w.shape[1] % 4 != 0:
            raise InvalidValue("weights dim 1 must be 4 * hidden_size")
        b, h0, c0 = _get(inputs, 3), _get(inputs, 5), _get(inputs, 6)
        if b is not None:
            _rnn_dims(b, 2, "bias")
            if b.shape[1] % 8 != 0:
                raise InvalidValue("bias dim 1 must be 8 * hidden_size")
        if h0 is not None:
            _rnn_dims(h0, 3, "initial_hidden")
        if c0 is not None:
            _rnn_dims(c0, 3, "initial_cell")
        return self._launch(ctx, "rten_hip_lstm_f32", x, [w, r, b, h0, c0], 3, outputs)


# ------------------------------------------------------------------------------------------ decoder blocks: RMS / skip normalisation, rotary embedding
SKIP_NORM_LAYER, SKIP_NORM_RMS = 0, 1  # RTEN_HIP_SKIP_NORM_*
ROTARY_POS_NONE, ROTARY_POS_IDS, ROTARY_POS_OFFSET = 0, 1, 2  # RTEN_HIP_ROTARY_POS_*


def _dense(ctx, x):
    """A contiguous DeviceTensor of a DeviceTensor or an einsum.View (re-laid when it is strided)."""
    from . import einsum as E
    return E.materialize(ctx, x) if isinstance(x, E.View) else x


def _one_element(t):
    """`scale.item()` of layer_normalization_impl (norm.rs:470): the value of a tensor of exactly one element, any rank; None otherwise.  A host array costs
    nothing; a device tensor is read back (constants of a graph are host values in the executor)."""
    if isinstance(t, DeviceTensor):
        return float(t.numpy().reshape(())) if t.size == 1 else None
    a = np.asarray(t)
    return float(a.reshape(())) if a.size == 1 else None


class RMSNormalization(Operator):
    """src/ops/norm.rs:419-435,571-608 (rten_hip_rms_norm_f32).  inputs: X, scale.  The slice shape[axis..] is normalised by its root mean square:
    y = x * (scale[i] * r), r = 1 / sqrt(SumSquare / n + epsilon); a one-element scale gives y = mul_add(x, scale / sqrt(..), 0).  Loader defaults
    (onnx_registry.rs:1584-1590): axis -1, epsilon absent = 1e-5, stash_type must be 1."""

    def __init__(self, axis=-1, epsilon=None):
        self.axis, self.epsilon = axis, epsilon

    def max_inputs(self):
        return 2

    def run(self, ctx, inputs):
        from . import einsum as E
        x = _require(inputs, 0)
        _want(x.t if isinstance(x, E.View) else x, np.float32)
        scale = _want(_require(inputs, 1), np.float32)
        x = _dense(ctx, x)  # (to_contiguous_in, norm.rs:497)
        ax = _resolve_axis(len(x.shape), self.axis)
        norm_shape = tuple(x.shape[ax:])
        cols = int(np.prod(norm_shape, dtype=np.int64))
        gamma, gs = None, _one_element(scale)
        if gs is None:
            if _broadcast_shapes(tuple(scale.shape), norm_shape) != norm_shape:
                raise InvalidValue("`scale` is not broadcastable to normalized axes of input")
            if scale.size != cols:
                raise UnsupportedValue("device path needs scale already expanded to the normalized shape")
            gamma = scale if isinstance(scale, DeviceTensor) else DeviceTensor.from_numpy(ctx, scale)
        y = DeviceTensor(ctx, x.shape, np.float32)
        if x.size:
            ctx.call("rten_hip_rms_norm_f32", x.size // cols, cols, x.vp, _vp(gamma), 1.0 if gs is None else gs, 1e-5 if self.epsilon is None else self.epsilon, y.vp)
        return [y]


class SimplifiedLayerNormalization(RMSNormalization):
    """src/ops/norm/contrib.rs:86-115: the contrib spelling of RMSNormalization, registered in ai.onnx (onnx_registry.rs:275,1905)."""


class _SkipNorm(Operator):
    """skip_layer_normalization, src/ops/norm/contrib.rs:22-77 (rten_hip_skip_norm_f32): sum = (input + skip) + bias, normalised over the last axis.
    `outputs` says which of (output, mean, inv_std_var, input_skip_bias_sum) a caller reads: the sum comes from the same launch when entry 3 is set; mean and
    inv_std_var are training outputs the reference fills with zeros, and asking for them here is UnsupportedValue.  Returns [output] or
    [output, None, None, sum]."""

    MODE = SKIP_NORM_LAYER

    def __init__(self, epsilon):
        self.epsilon = epsilon

    def max_outputs(self):
        return 4

    def _operands(self, inputs):
        raise NotImplementedError

    def run(self, ctx, inputs, outputs=None):
        x = _dense(ctx, _require(inputs, 0))
        skip = _dense(ctx, _require(inputs, 1))
        _want(x, np.float32), _want(skip, np.float32)
        gamma, beta, bias = self._operands(inputs)
        for t in (gamma, beta, bias):
            if t is not None:
                _want(t, np.float32)
                if len(t.shape) != 1:
                    raise OpError("InputCastFailed", "expected tensor with 1 dims")
        want = list(outputs) + [False] * (4 - len(outputs)) if outputs is not None else [True, False, False, False]
        if want[1] or want[2]:
            raise UnsupportedValue("the mean and inv_std_var outputs are not computed")
        if len(x.shape) not in (2, 3):
            raise InvalidValue("input must be 2 or 3 dimensioned")
        if len(skip.shape) not in (2, 3):
            raise InvalidValue("skip must be 2 or 3 dimensioned")
        if tuple(skip.shape[-2:]) != tuple(x.shape[-2:]) or (len(skip.shape) == 3 and skip.shape[0] not in (1, x.shape[0])) or len(skip.shape) > len(x.shape):
            raise IncompatibleInputShapes("skip must broadcast to input over the batch dimension")
        cols = x.shape[-1]
        if bias is not None and bias.shape[0] not in (1, cols):
            raise IncompatibleInputShapes("Cannot broadcast inputs")  # (add_in_place, binary_elementwise.rs)
        one = _one_element(gamma) is not None
        if not one and gamma.shape[0] != cols:
            raise InvalidValue("`scale` is not broadcastable to normalized axes of input")
        if beta is not None and beta.shape[0] not in (1, cols):
            raise InvalidValue("`bias` is not broadcastable to normalized axes of input")
        y = DeviceTensor(ctx, x.shape, np.float32)
        total = DeviceTensor(ctx, x.shape, np.float32) if want[3] else None
        if x.size:
            if one or (bias is not None and bias.shape[0] != cols) or (beta is not None and beta.shape[0] != cols):
                # a one-element gamma is the reference's scalar scale (other bits than a vector of equal values), a one-element bias / beta a broadcast: the
                # operators one after the other, on the entry points that take a scalar
                s = Add().run(ctx, [x, skip])[0]
                if bias is not None:
                    s = Add().run(ctx, [s, bias])[0]
                norm = RMSNormalization(-1, self.epsilon) if self.MODE == SKIP_NORM_RMS else LayerNormalization(-1, self.epsilon)
                scale = gamma.reshape(()) if one else gamma
                y = norm.run(ctx, [s, scale] + ([beta.reshape(()) if beta.shape[0] == 1 else beta] if beta is not None else []))[0]
                total = s if want[3] else None
            else:
                ctx.call("rten_hip_skip_norm_f32", self.MODE, x.size // cols, cols, x.vp, skip.vp, skip.size // cols, _vp(bias), gamma.vp, _vp(beta), self.epsilon,
                         _vp(total), y.vp)
        return [y, None, None, total] if want[3] else [y]


class SkipLayerNormalization(_SkipNorm):
    """com.microsoft, src/ops/norm/contrib.rs:123-177.  inputs: input, skip, gamma, beta?, bias?; `epsilon` is required (onnx_registry.rs:1918-1922)."""

    def max_inputs(self):
        return 5

    def _operands(self, inputs):
        return _require(inputs, 2), _get(inputs, 3), _get(inputs, 4)


class SkipSimplifiedLayerNormalization(_SkipNorm):
    """com.microsoft, src/ops/norm/contrib.rs:186-238: the RMS form.  inputs: input, skip, gamma, bias?."""

    MODE = SKIP_NORM_RMS

    def name(self):
        return "SkipSimplifiedLayerNormalisation"  # (sic, contrib.rs:192)

    def max_inputs(self):
        return 4

    def _operands(self, inputs):
        return _require(inputs, 2), None, _get(inputs, 3)


def rotary_cache_dims(cache_shape, batch, seq_len, half, bad_last_dim):
    """src/ops/embedding.rs:20-44: a cos / sin cache is [1 | batch, 1 | seq_len, rotary_embedding_dim / 2]; returns its (batch, seq_len) dims."""
    if len(cache_shape) != 3:
        raise InvalidValue("cos/sin cache must be a 3D tensor")
    cache_batch, cache_seq, cache_half = cache_shape
    if cache_half != half:
        raise InvalidValue(bad_last_dim)
    if cache_seq != 1 and cache_seq != seq_len:
        raise InvalidValue("cos/sin cache sequence length must be 1 or match the input")
    if cache_batch != 1 and cache_batch != batch:
        raise InvalidValue("cos/sin cache batch size must be 1 or match the input")
    return cache_batch, cache_seq


def _host_ids(t):
    """position_ids known on the host (a numpy array or a Python int; the loader narrows int64 to int32) as an int32 array; None for device data."""
    if isinstance(t, DeviceTensor):
        return None
    a = np.asarray(t)
    if a.dtype.kind not in "iu":
        raise OpError("InputCastFailed", "expected int32 tensor")
    return a.astype(np.int32)


def rotary_embedding(ctx, x, cos, sin, position_ids, offset, interleaved, num_heads, rotary_embedding_dim):
    """rotary_embedding, src/ops/embedding.rs:46-207 (rten_hip_rotary_embedding_f32).  `x` may be an einsum.View with a unit stride along its last axis --
    a q or k column block of a fused projection -- and is then read in place.  `position_ids`: int32 [batch, seq] ids, or, with `offset`, the contrib
    operator's one-element offset k (token i uses position k + i); a DeviceTensor is gathered by the kernel (an id outside the cache is clamped as Gather on
    device data is), a host array is checked here."""
    from . import einsum as E
    _want(x.t if isinstance(x, E.View) else x, np.float32)
    v = x if isinstance(x, E.View) else E.View(x)
    if len(v.shape) in (3, 4) and v.shape[-1] > 1 and v.strides[-1] != 1:
        v = E.View(E.materialize(ctx, v))  # (to_contiguous_in, embedding.rs:128-131)
    if len(v.shape) == 3:
        batch, seq_len, hidden = v.shape
        if num_heads == 0:
            raise InvalidValue("num_heads must not be 0 for 3 dimensioned input")
        if hidden % num_heads != 0:
            raise InvalidValue("hidden_size must be divisible by num_heads")
        heads, head_size = num_heads, hidden // num_heads
        xst = (v.strides[0], v.strides[1], head_size)
        yst = (seq_len * hidden, hidden, head_size)
    elif len(v.shape) == 4:
        batch, heads, seq_len, head_size = v.shape
        xst = (v.strides[0], v.strides[2], v.strides[1])
        yst = (heads * seq_len * head_size, head_size, seq_len * head_size)
    else:
        raise IncompatibleInputShapes("Input processed needs 3-4 dimensions")
    rot = head_size if rotary_embedding_dim == 0 else rotary_embedding_dim
    if rot == 0 or rot % 2 != 0:
        raise InvalidValue("rotary_embedding_dim must be a positive even number")
    if rot > head_size:
        raise InvalidValue("rotary_embedding_dim must not exceed head size")
    half = rot // 2
    cos, sin = _dense(ctx, cos), _dense(ctx, sin)
    _want(cos, np.float32), _want(sin, np.float32)
    mode, max_pos, ids, cst, sst = ROTARY_POS_NONE, 0, None, (0, 0), (0, 0)
    if position_ids is not None:
        host = _host_ids(position_ids)
        if host is None:
            _want(position_ids, np.int32)
        id_shape = (batch, seq_len) if offset else tuple(position_ids.shape if host is None else host.shape)
        # gather(cos, 0, ids) has shape ids.shape + cos.shape[1..]
        for cache, msg in ((cos, "Last dimension of cos cache does not match rotary_embedding_dim/2"), (sin, "Last dimension of sin cache does not match rotary_embedding_dim/2")):
            if len(cache.shape) == 0:
                raise InvalidValue("Cannot gather from a scalar")  # (gather.rs)
            rotary_cache_dims(id_shape + tuple(cache.shape[1:]), batch, seq_len, half, msg)
        if cos.shape[0] != sin.shape[0]:
            raise UnsupportedValue("device path needs cos and sin caches of one length")
        max_pos = cos.shape[0]
        if host is not None:
            pos = host.reshape(-1)[:1].astype(np.int64) + np.arange(seq_len) if offset else host.astype(np.int64)
            if pos.size and (pos.min() < -max_pos or pos.max() >= max_pos):
                raise InvalidValue("Entry in `indices` is out of range")
            if not offset:
                host = np.ascontiguousarray(np.broadcast_to(host, (batch, seq_len)))
            ids = DeviceTensor.from_numpy(ctx, host.reshape(-1)[:1] if offset else host)
        else:
            if not offset and id_shape != (batch, seq_len):
                raise UnsupportedValue("device position_ids must have the input's [batch, seq] shape")
            ids = position_ids
        mode = ROTARY_POS_OFFSET if offset else ROTARY_POS_IDS
    else:
        cb, cs = rotary_cache_dims(tuple(cos.shape), batch, seq_len, half, "Last dimension of cos cache does not match rotary_embedding_dim/2")
        sb, ss = rotary_cache_dims(tuple(sin.shape), batch, seq_len, half, "Last dimension of sin cache does not match rotary_embedding_dim/2")
        cst = (0 if cb == 1 else cs * half, 0 if cs == 1 else half)
        sst = (0 if sb == 1 else ss * half, 0 if ss == 1 else half)
    y = DeviceTensor(ctx, v.shape, np.float32)
    if y.size:
        ctx.call("rten_hip_rotary_embedding_f32", batch, seq_len, heads, head_size, rot, 1 if interleaved else 0, v.t.vp, *xst, cos.vp, *cst, sin.vp, *sst,
                 _vp(ids), mode, max_pos, y.vp, *yst)
    return y


class RotaryEmbedding(Operator):
    """ai.onnx, src/ops/embedding.rs:209-252.  inputs: X [B, S, H * D] (needs num_heads) or [B, H, S, D], cos, sin, position_ids [B, S]?.  Loader defaults
    (onnx_registry.rs:1832-1847): interleaved false, num_heads 0, rotary_embedding_dim 0 (= head size)."""

    def __init__(self, interleaved=False, num_heads=0, rotary_embedding_dim=0):
        self.interleaved, self.num_heads, self.rotary_embedding_dim = bool(interleaved), num_heads, rotary_embedding_dim

    def max_inputs(self):
        return 4

    def run(self, ctx, inputs):
        x, cos, sin, ids = _require(inputs, 0), _require(inputs, 1), _require(inputs, 2), _get(inputs, 3)
        if ids is not None and len(np.shape(ids) if not isinstance(ids, DeviceTensor) else ids.shape) != 2:
            raise OpError("InputCastFailed", "expected tensor with 2 dims")
        return [rotary_embedding(ctx, x, cos, sin, ids, False, self.interleaved, self.num_heads, self.rotary_embedding_dim)]


class RotaryEmbeddingMicrosoft(Operator):
    """com.microsoft RotaryEmbedding, src/ops/embedding/contrib.rs:17-135.  inputs: X, position_ids, cos [max_pos, half], sin.  position_ids is [B, S], or a
    scalar / one-element vector holding an offset k (token i uses position k + i).  num_heads 0 or None is inferred from the cache for a 3-D input, which
    rotary_embedding_dim != 0 rules out."""

    def __init__(self, interleaved=False, num_heads=None, rotary_embedding_dim=0):
        self.interleaved, self.num_heads, self.rotary_embedding_dim = bool(interleaved), num_heads, rotary_embedding_dim

    def name(self):
        return "com.microsoft.RotaryEmbedding"

    def max_inputs(self):
        return 4

    def run(self, ctx, inputs):
        from . import einsum as E
        x, ids, cos, sin = (_require(inputs, i) for i in range(4))
        xs = tuple(x.shape)
        if len(xs) not in (3, 4):
            raise IncompatibleInputShapes("Input processed needs 3-4 dimensions")
        ids_shape = tuple(ids.shape) if isinstance(ids, DeviceTensor) else np.shape(ids)
        n_ids = int(np.prod(ids_shape, dtype=np.int64))
        if len(ids_shape) in (0, 1) and n_ids == 1:
            offset = True
        elif len(ids_shape) == 2:
            offset = False
        else:
            raise InvalidValue("position_ids must be a scalar, a 1-element vector or have 2 dims")
        num_heads = self.num_heads or 0
        if len(xs) == 3 and num_heads == 0:
            if self.rotary_embedding_dim != 0:
                raise InvalidValue("num_heads must be specified when rotary_embedding_dim is set")
            if len(cos.shape) == 0:
                raise InvalidValue("cos cache must not be scalar")
            if cos.shape[-1] == 0:
                raise InvalidValue("Last dimension of cos cache must not be 0")
            head_size = cos.shape[-1] * 2
            if xs[2] % head_size != 0:
                raise InvalidValue("hidden_size must be divisible by head size")
            num_heads = xs[2] // head_size
        return [rotary_embedding(ctx, x, cos, sin, ids, offset, self.interleaved, num_heads, self.rotary_embedding_dim)]


def _shape_of(t):
    return tuple(t.shape) if isinstance(t, DeviceTensor) else tuple(np.shape(t))


def _int32_operand(ctx, t):
    """An int32 input that may arrive as a host value (numpy / int: validated by the caller, then uploaded) or as device data -> (host array | None, DeviceTensor)."""
    if isinstance(t, DeviceTensor):
        return None, _want(t, np.int32)
    a = np.asarray(t)
    if a.dtype.kind not in "iu":
        raise OpError("InputCastFailed", "expected int32 tensor")
    a = np.ascontiguousarray(a.astype(np.int32))
    return a, DeviceTensor.from_numpy(ctx, a.reshape(-1))


class GroupQueryAttention(Operator):
    """com.microsoft.GroupQueryAttention with a KV cache, src/ops/attention/contrib.rs:419-878 (rten_hip_gqa_f32: one prepare-and-append launch, then the
    one-launch decode kernel or GEMM, score kernel, GEMM).  inputs: query [B, S, H * D] (packed [B, S, (H + 2 KV) * D] with key and value absent), key,
    value [B, S, KV * D], past_key, past_value [B, KV, P, D], seqlens_k int32 [B] or [B, 1], total_sequence_length int32 scalar, cos_cache, sin_cache
    [max, rot / 2], position_ids int32 [B, S], attention_bias [B | 1, H | 1, >= S, >= P + S], head_sink (refused).  query may be an einsum.View with a unit
    stride along its last axis (a fused projection's column block), read in place.
    Loader defaults (onnx_registry.rs:1467-1492): scale None (1 / sqrt(D)), do_rotary, rotary_interleaved and smooth_softmax false, local_window_size -1 (a
    non-positive size disables the window), softcap 0.
    seqlens_k and total_sequence_length that arrive as host values are validated here with the reference's errors (contrib.rs:582-639); DeviceTensors stay on
    the device, where the kernels clamp kv_len into [1, P + S] and past_len into [0, P] instead.  `outputs`: the requested output indices; present_key /
    present_value are RETURNED only when 1 or 2 is among them (contrib.rs:803-807) -- they are always computed, because the attention kernels read K and V
    out of them.
    Not built: softcap != 0 (the reference calls libm's tanh there), smooth_softmax, head_sink."""

    def __init__(self, num_heads, kv_num_heads, scale=None, do_rotary=False, rotary_interleaved=False, local_window_size=-1, softcap=0.0, smooth_softmax=False):
        self.num_heads, self.kv_num_heads, self.scale = int(num_heads), int(kv_num_heads), scale
        self.do_rotary, self.rotary_interleaved = bool(do_rotary), bool(rotary_interleaved)
        lw = -1 if local_window_size is None else int(local_window_size)
        self.local_window_size = lw if lw > 0 else None
        self.softcap, self.smooth_softmax = float(softcap), bool(smooth_softmax)

    def name(self):
        return "com.microsoft.GroupQueryAttention"

    def max_inputs(self):
        return 12

    def max_outputs(self):
        return 3

    def run(self, ctx, inputs, outputs=(0, 1, 2)):
        from . import einsum as E
        query = _require(inputs, 0)
        qv = query if isinstance(query, E.View) else E.View(query)
        _want(qv.t, np.float32)
        if len(qv.shape) != 3:
            raise OpError("InputCastFailed", "expected tensor with 3 dims")
        if qv.shape[-1] > 1 and qv.strides[-1] != 1:
            qv = E.View(E.materialize(ctx, qv))
        key, value = _get(inputs, 1), _get(inputs, 2)
        past_key, past_value = _get(inputs, 3), _get(inputs, 4)
        seqlens, total = _require(inputs, 5), _require(inputs, 6)
        cos, sin, position_ids, bias, head_sink = (_get(inputs, i) for i in range(7, 12))
        for t in (key, value):
            if t is not None:
                _want(t, np.float32)
                if len(t.shape) != 3:
                    raise OpError("InputCastFailed", "expected tensor with 3 dims")
        sl_shape = list(_shape_of(seqlens))
        while len(sl_shape) > 1 and sl_shape[-1] == 1:
            sl_shape.pop()
        if len(sl_shape) != 1:
            raise UnsupportedValue("seqlens_k must be a vector")
        if len(_shape_of(total)) != 0 and not (isinstance(total, DeviceTensor) and total.size == 1):
            raise OpError("InputCastFailed", "expected tensor with 0 dims")
        if head_sink is not None:
            raise UnsupportedValue("head_sink is not supported")
        if self.smooth_softmax:
            raise UnsupportedValue("smooth_softmax is not supported")
        H, KV = self.num_heads, self.kv_num_heads
        if H <= 0 or KV <= 0:
            raise InvalidValue("num_heads and kv_num_heads must be positive")
        if H % KV != 0:
            raise InvalidValue("num_heads must be a multiple of kv_num_heads")
        batch, seq, q_hidden = qv.shape
        qb = qv.t.ptr
        if key is not None and value is not None:
            if q_hidden % H != 0:
                raise IncompatibleInputShapes("query hidden size must be divisible by num_heads")
            D = q_hidden // H
            key, value = _dense(ctx, key), _dense(ctx, value)
            if key.shape[0] != batch or value.shape[0] != batch:
                raise IncompatibleInputShapes("key and value batch size must match query")
            if tuple(key.shape[1:]) != tuple(value.shape[1:]):
                raise IncompatibleInputShapes("key and value must have the same shape")
            if key.shape[2] != KV * D:
                raise IncompatibleInputShapes("key hidden size must equal kv_num_heads * head_size")
            if key.shape[1] != seq:
                raise UnsupportedValue("key sequence length must match query sequence length")
            ptrs = (qb, key.ptr, value.ptr)
            kvst = (seq * KV * D, KV * D, D)
            strides = [qv.strides[0], qv.strides[1], D, *kvst, *kvst]
        elif key is None and value is None:
            if q_hidden % (H + 2 * KV) != 0:
                raise IncompatibleInputShapes("packed query hidden size must be divisible by num_heads + 2 * kv_num_heads")
            D = q_hidden // (H + 2 * KV)
            ptrs = (qb, qb + 4 * H * D, qb + 4 * (H + KV) * D)
            strides = [qv.strides[0], qv.strides[1], D] * 3
        else:
            raise InvalidValue("key and value must both be present or both absent")
        if sl_shape[0] != batch:
            raise IncompatibleInputShapes("seqlens_k must have batch_size elements")
        total_host, total_dev = _int32_operand(ctx, total)
        if total_host is not None and int(total_host.reshape(())) <= 0:
            raise InvalidValue("total_sequence_length must be positive")
        if past_key is not None and past_value is not None:
            past_key, past_value = _dense(ctx, _want(past_key, np.float32)), _dense(ctx, _want(past_value, np.float32))
            if len(past_key.shape) != 4 or len(past_value.shape) != 4:
                raise OpError("InputCastFailed", "expected tensor with 4 dims")
            if tuple(past_key.shape) != tuple(past_value.shape) or tuple(past_key.shape[:2]) != (batch, KV) or past_key.shape[3] != D:
                raise IncompatibleInputShapes("past_key/past_value shape does not match")
            past_seq = past_key.shape[2]
        elif past_key is None and past_value is None:
            past_seq = 0
        else:
            raise InvalidValue("past_key and past_value must both be present or both absent")
        present_seq = past_seq + seq
        seqlens_host, seqlens_dev = _int32_operand(ctx, seqlens)
        if total_host is not None:
            tot = int(total_host.reshape(()))
            first, subsequent = seq == tot, seq > 1 and seq != tot
            if subsequent and batch != 1:
                raise UnsupportedValue("batch size must be 1 when sequence_length > 1 and a past context is given")
            if not first and not subsequent and seq != 1:
                raise InvalidValue("sequence_length must be 1 when query is not a prompt")
        if seqlens_host is not None:
            for n in seqlens_host.reshape(-1):
                if n < 0 or n >= present_seq:
                    raise InvalidValue("seqlens_k entry is out of range")
                if n + 1 < seq:
                    raise InvalidValue("seqlens_k entry is too small for the query sequence length")
        bias_strides = [0, 0, 0]
        if bias is not None:
            bias = _dense(ctx, _want(bias, np.float32))
            if len(bias.shape) != 4:
                raise OpError("InputCastFailed", "expected tensor with 4 dims")
            bb, bh, bs, bt = bias.shape
            if (bb != 1 and bb != batch) or (bh != 1 and bh != H) or bs < seq or bt < present_seq:
                raise IncompatibleInputShapes("attention_bias shape is incompatible with query/key shapes")
            bias_strides = [0 if bb == 1 else bh * bs * bt, 0 if bh == 1 else bs * bt, bt]
        scale = self.scale
        if scale is None:
            scale = float(np.float32(1.0) / np.sqrt(np.float32(D))) if D else 0.0
        rot, max_pos = 0, 0
        if self.do_rotary:
            if cos is None or sin is None:
                raise InvalidValue("cos_cache and sin_cache are required when do_rotary is set")
            cos, sin = _dense(ctx, _want(cos, np.float32)), _dense(ctx, _want(sin, np.float32))
            if len(cos.shape) != 2 or len(sin.shape) != 2:
                raise OpError("InputCastFailed", "expected tensor with 2 dims")
            rot = 2 * cos.shape[1]
            if rot == 0 or rot % 2 != 0:
                raise InvalidValue("rotary_embedding_dim must be a positive even number")
            if rot > D:
                raise InvalidValue("rotary_embedding_dim must not exceed head size")
            if sin.shape[1] != cos.shape[1]:
                raise InvalidValue("Last dimension of sin cache does not match rotary_embedding_dim/2")
            if cos.shape[0] != sin.shape[0]:
                raise UnsupportedValue("device path needs cos and sin caches of one length")
            max_pos = cos.shape[0]
            if position_ids is not None:
                ids_host, position_ids = _int32_operand(ctx, position_ids)
                if ids_host is not None:
                    if ids_host.ndim != 2:
                        raise OpError("InputCastFailed", "expected tensor with 2 dims")
                    if ids_host.shape[1] not in (1, seq):
                        raise InvalidValue("cos/sin cache sequence length must be 1 or match the input")
                    if ids_host.shape[0] not in (1, batch):
                        raise InvalidValue("cos/sin cache batch size must be 1 or match the input")
                    if ids_host.size and (ids_host.min() < -max_pos or ids_host.max() >= max_pos):
                        raise InvalidValue("Entry in `indices` is out of range")
                    position_ids = DeviceTensor.from_numpy(ctx, np.ascontiguousarray(np.broadcast_to(ids_host, (batch, seq))))
                elif tuple(position_ids.shape) != (batch, seq):
                    raise UnsupportedValue("device position_ids must have the input's [batch, seq] shape")
            elif seqlens_host is not None and total_host is not None and max_pos > 0:
                tot = int(total_host.reshape(()))
                last = seq - 1 if seq == tot else int(seqlens_host.max(initial=0))
                if last >= max_pos:
                    raise InvalidValue("Entry in `indices` is out of range")
        else:
            cos = sin = position_ids = None
        if self.softcap != 0.0:
            raise UnsupportedValue("softcap is not supported")
        out = DeviceTensor(ctx, (batch, seq, H * D), np.float32)
        present_key = DeviceTensor(ctx, (batch, KV, present_seq, D), np.float32)
        present_value = DeviceTensor(ctx, (batch, KV, present_seq, D), np.float32)
        if out.size and KV * D:
            dims = (C.c_int32 * L.GQA_NDIMS)(batch, seq, H, KV, D, past_seq, rot, 1 if self.rotary_interleaved else 0, max_pos, self.local_window_size or 0)
            st = (C.c_int64 * L.GQA_NSTRIDES)(*strides, *bias_strides)
            ctx.call("rten_hip_gqa_f32", dims, st, scale, *(C.c_void_p(p) for p in ptrs), _vp(past_key), _vp(past_value), seqlens_dev.vp, total_dev.vp,
                     _vp(cos), _vp(sin), _vp(position_ids) if self.do_rotary else None, _vp(bias), out.vp, present_key.vp, present_value.vp)
        if 1 in outputs or 2 in outputs:
            return [out, present_key, present_value]
        return [out]


class OpRegistry:
    """Mirror of OpRegistry (src/op_registry.rs:25-72): op_type -> operator class for the hot path."""

    def __init__(self):
        self._ops = {}

    @classmethod
    def with_all_ops(cls):
        r = cls()
        for op in (Conv, ConvTranspose, ConvInteger, ConvIntegerToFloat, MatMul, FusedMatMul, Gemm, MatMulInteger, MatMulIntegerToFloat, MatMulNBits,
                   Softmax, LogSoftmax, AddSoftmax, LayerNormalization, BatchNormalization, InstanceNormalization, Relu, Gelu, Erf, Add, Mul, Sub, Div, Transpose, MaxPool,
                   AveragePool, GlobalAveragePool, Flatten, DynamicQuantizeLinear, Attention, Gather, ReduceSum, ReduceMean, Einsum, Resize, Upsample,
                   Split, ReduceMax, ReduceMin, ArgMax, ArgMin, TopK, GRU, LSTM, Neg, Abs, Sign, Floor, Ceil, Round, Sqrt, Reciprocal, Exp, Log, Softplus,
                   Pow, PRelu, Min, Max, Sum, Mean, Pad, QuantizeLinear, DequantizeLinear, ReduceL1, ReduceL2, ReduceSumSquare, ReduceLogSum, ReduceLogSumExp,
                   ReduceProd, LpNormalization, GlobalMaxPool, GridSample, DepthToSpace, CumSum, GatherElements, Trilu, Tile,
                   NonMaxSuppression, DFT, STFT, RMSNormalization, SimplifiedLayerNormalization, SkipLayerNormalization,
                   SkipSimplifiedLayerNormalization, RotaryEmbedding, RotaryEmbeddingMicrosoft, GroupQueryAttention):
            r.register_op(op)
        return r

    def register_op(self, op_cls):
        self._ops[op_cls.__name__] = op_cls

    def get(self, op_type: str):
        return self._ops.get(op_type)

    def op_types(self):
        return sorted(self._ops)
