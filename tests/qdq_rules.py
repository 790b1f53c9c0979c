"""QuantizeLinear / DequantizeLinear as the reference computes them (src/ops/quantize.rs:19-334, rten-vecmath/src/quantize.rs), restated in numpy.

The expected values of tests/test_qdq_ops.py and tests/test_gpu_qdq.py come from here.  Every f32 operation below is one IEEE operation on float32 arrays
(numpy rounds each correctly), so the results are the reference's bits.

The reference has several code paths for QuantizeLinear:
  * per-tensor u8 on contiguous data: rten-vecmath's kernel, `quantize_u8_chunked` (64-element AVX-512 chunks, then a scalar tail);
  * every other form (i8; per-axis; non-contiguous): the scalar definition `Quantize::quantize`, `quantize_scalar`.
They compute the same function wherever round(x * inv_scale) + zero_point fits in an i32 and x * inv_scale is finite (in particular for every
|x * inv_scale| < 2^31 - 255); outside they disagree with each other.  `quantize_linear` is the device's documented choice (docs/KERNELS.md 4.9):
u8 per-tensor follows `quant_u8_rule` (the statement of the vector kernel the int8 path already uses), everything else the scalar definition."""
import numpy as np

F32 = np.float32
LIMITS = {np.dtype(np.uint8): (0, 255), np.dtype(np.int8): (-128, 127)}


class RuleError(Exception):
    def __init__(self, kind, msg=""):
        super().__init__(f"{kind}({msg!r})")
        self.kind, self.msg = kind, msg


def inv_scale_of(scale):
    """quantize.rs:210,262: one correctly rounded f32 division."""
    with np.errstate(divide="ignore"):
        return (F32(1.0) / np.asarray(scale, F32)).astype(F32)


def _saturating_cast(y, dtype):
    """Rust `f32 as u8 / i8 / i32`: NaN -> 0, otherwise clamp and truncate."""
    info = np.iinfo(dtype)
    y = np.asarray(y, F32)
    out = np.zeros(y.shape, np.int64)
    ok = ~np.isnan(y)
    out[ok] = np.trunc(np.clip(y[ok].astype(np.float64), info.min, info.max)).astype(np.int64)
    return out.astype(dtype)


def _wrap32(v):
    return ((np.asarray(v, np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int64)


def quantize_scalar(x, inv_scale, zp, dtype):
    """Quantize::quantize (quantize.rs:171-194): (x * inv_scale).round_ties_even() + zp as f32, then a saturating cast."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        y = np.rint((x * F32(inv_scale)).astype(F32)).astype(F32)
        y = (y + F32(int(zp))).astype(F32)
    return _saturating_cast(y, dtype)


def _to_int_round(p):
    """cvtps2dq: round to nearest even; NaN and values outside i32 give the "integer indefinite" i32::MIN."""
    p = np.asarray(p, F32)
    with np.errstate(all="ignore"):
        r = np.rint(p).astype(np.float64)
    bad = np.isnan(r) | (r >= 2.0 ** 31) | (r < -(2.0 ** 31))
    out = np.where(bad, -(2.0 ** 31), r)
    return out.astype(np.int64)


def quantize_u8_chunked(x, inv_scale, zp, lanes=64):
    """rten-vecmath/src/quantize.rs:38-77 with AVX-512 (16 f32 lanes x 4 vectors = 64 elements per chunk): to_int_round, a wrapping i32 add of the zero
    point, saturating narrowing i32 -> i16 -> u8; the remainder goes through the scalar tail (a saturating `as i32`, a wrapping add, clamp)."""
    x = np.asarray(x, F32).ravel()
    n_vec = len(x) // lanes * lanes
    out = np.empty(len(x), np.uint8)
    with np.errstate(all="ignore"):
        p = (x * F32(inv_scale)).astype(F32)
    q = _wrap32(_to_int_round(p[:n_vec]) + int(zp))
    q = np.clip(q, -32768, 32767)  # i32 -> i16, signed saturation
    out[:n_vec] = np.clip(q, 0, 255).astype(np.uint8)  # i16 -> u8, unsigned saturation
    with np.errstate(all="ignore"):
        t = _saturating_cast(np.rint(p[n_vec:]).astype(F32), np.int32).astype(np.int64)
    out[n_vec:] = np.clip(_wrap32(t + int(zp)), 0, 255).astype(np.uint8)
    return out


def quant_u8_rule(x, inv_scale, zp):
    """dql::quant_u8 (rten_amd/csrc/quantize.h), the device's statement of the vector kernel: the product is clamped to +-1024 (NaN -> the lower bound),
    a product >= 2^31 goes to the lower bound too (cvtps2dq's i32::MIN), then round, add, clamp to 0..255."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        p = (x * F32(inv_scale)).astype(F32)
    pc = np.where(np.isnan(p), F32(-1024.0), np.clip(p, F32(-1024.0), F32(1024.0))).astype(F32)
    pc = np.where(p >= F32(2147483648.0), F32(-1024.0), pc)
    return np.clip(np.rint(pc).astype(np.int64) + int(zp), 0, 255).astype(np.uint8)


def geometry(shape, scale_shape, zp_shape, axis, what):
    """-> (outer, channels, inner) and whether the form is per-tensor; the reference's checks in the reference's order (quantize.rs:41-99,196-275).
    `what`: "quantization" / "dequantization".  The per-axis zero-point length check is DequantizeLinear's; QuantizeLinear applies it too (the one
    deviation: the reference's zip is cut short there)."""
    shape = tuple(int(d) for d in shape)
    n = int(np.prod(shape, dtype=np.int64))
    if int(np.prod(scale_shape, dtype=np.int64)) == 1:
        if zp_shape is not None and int(np.prod(zp_shape, dtype=np.int64)) != 1:
            raise RuleError("InvalidValue", "scale and zero_point must have same shape")
        return (1, 1, n), True
    if len(scale_shape) != 1:
        raise RuleError("UnsupportedValue", f"Blocked {what} is not supported")
    if axis < -len(shape) or axis >= len(shape):
        raise RuleError("InvalidValue", "Axis is invalid")
    ax = axis % len(shape)
    if scale_shape[0] != shape[ax]:
        raise RuleError("IncompatibleInputShapes", "scale length does not match size of quantization axis")
    if zp_shape is not None:
        if len(zp_shape) != 1:
            raise RuleError("InvalidValue", "scale and zero point must have same rank" if what == "dequantization" else "scale and zero point must have same shape")
        if zp_shape[0] != shape[ax]:
            raise RuleError("IncompatibleInputShapes", "zero_point length does not match size of quantization axis")
    return (int(np.prod(shape[:ax], dtype=np.int64)), shape[ax], int(np.prod(shape[ax + 1:], dtype=np.int64))), False


def output_dtype(zero_point, attr_dtype):
    """quantize.rs:299-323."""
    u8, i8 = np.dtype(np.uint8), np.dtype(np.int8)
    attr = None if attr_dtype is None else np.dtype(attr_dtype)
    if zero_point is not None:
        zd = np.asarray(zero_point).dtype
        if zd in (u8, i8) and attr in (None, zd):
            return zd
    elif attr in (u8, i8):
        return attr
    raise RuleError("UnsupportedType")


def quantize_linear(x, scale, zero_point=None, axis=-1, dtype=None, u8_per_tensor=quant_u8_rule):
    """The device's QuantizeLinear.  `u8_per_tensor`: the rule of the per-tensor u8 form (quant_u8_rule; quantize_u8_chunked and quantize_scalar give
    the same codes inside the contract domain)."""
    x = np.asarray(x, F32)
    scale = np.asarray(scale, F32)
    dt = output_dtype(zero_point, dtype)
    zp = None if zero_point is None else np.asarray(zero_point)
    (outer, channels, inner), per_tensor = geometry(x.shape, scale.shape, None if zp is None else zp.shape, axis, "quantization")
    if x.size == 0:
        return np.zeros(x.shape, dt)
    if per_tensor:
        inv, z = inv_scale_of(scale.reshape(-1)[0]), 0 if zp is None else int(zp.reshape(-1)[0])
        if dt == np.uint8:
            return np.asarray(u8_per_tensor(x.ravel(), inv, z)).reshape(x.shape)
        return quantize_scalar(x, inv, z, dt)
    xv = x.reshape(outer, channels, inner)
    out = np.empty(xv.shape, dt)
    for c in range(channels):
        out[:, c, :] = quantize_scalar(xv[:, c, :], inv_scale_of(scale[c]), 0 if zp is None else int(zp[c]), dt)
    return out.reshape(x.shape)


def dequantize_linear(x, scale, zero_point=None, axis=1):
    """(x as i32 - zp as i32) as f32 * scale (quantize.rs:25-39); the i32 subtraction wraps for int32 inputs (a Rust release build)."""
    x = np.asarray(x)
    if x.dtype not in (np.dtype(np.uint8), np.dtype(np.int8), np.dtype(np.int32)):
        raise RuleError("UnsupportedType")
    scale = np.asarray(scale, F32)
    zp = None if zero_point is None else np.asarray(zero_point)
    (outer, channels, inner), per_tensor = geometry(x.shape, scale.shape, None if zp is None else zp.shape, axis, "dequantization")
    if x.size == 0:
        return np.zeros(x.shape, F32)
    if per_tensor:
        z = 0 if zp is None else int(zp.reshape(-1)[0])
        return (_wrap32(x.astype(np.int64) - z).astype(np.int32).astype(F32) * scale.reshape(-1)[0]).astype(F32)
    xv = x.reshape(outer, channels, inner).astype(np.int64)
    z = np.zeros(channels, np.int64) if zp is None else zp.astype(np.int64)
    d = _wrap32(xv - z[None, :, None]).astype(np.int32).astype(F32)
    return (d * scale[None, :, None]).astype(F32).reshape(x.shape)


def quantize_dequantize(x, scale, zero_point=None, axis=-1, dtype=None):
    """The round trip: QuantizeLinear then DequantizeLinear with the same parameters (what the executor's fused step computes)."""
    q = quantize_linear(x, scale, zero_point, axis, dtype)
    scale = np.asarray(scale, F32)
    return dequantize_linear(q, scale, zero_point, axis if scale.size != 1 else 1)
