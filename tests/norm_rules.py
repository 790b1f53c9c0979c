"""Expected values for InstanceNormalization, LogSoftmax and BatchNormalization (+ activation), built on the CPU oracle.

instance_norm: the reference normalises each (batch, channel) slice with the statistics LayerNormalization computes over a row and a
scalar scale / bias (src/ops/norm.rs:103-189,332-365), so a slice IS ref.layer_norm of a one-row matrix with gamma_scalar / beta_scalar.
log_softmax: rten-vecmath/src/softmax.rs:131-174 -- max, the sum of ReducedRangeExp(x - max) in the 16-lane single-accumulator order of
rto_softmax_row, y = (x - max) - ln(sum) as two subtractions; ln(sum) is the float64 logarithm rounded to float32 (the reference calls
the host's logf; `ln` lets a test substitute it)."""
import ctypes as C
import math

import numpy as np

from oracle import ref

F = np.float32
LANES = 16

ref.lib().rto_exp_reduced_f32.restype = C.c_float
ref.lib().rto_exp_reduced_f32.argtypes = [C.c_float]


def instance_norm(x, scale, bias, eps=1e-5):
    x = np.ascontiguousarray(x, np.float32)
    n, c = x.shape[:2]
    rows = x.reshape(n * c, -1)
    y = np.empty_like(rows)
    for r in range(n * c):
        ch = r % c
        y[r] = ref.layer_norm(rows[r][None, :], gamma_scalar=float(scale[ch]), beta_scalar=float(bias[ch]), eps=eps)[0]
    return y.reshape(x.shape)


def batch_norm(x, scale, bias, mean, var, eps=1e-5):
    x = np.asarray(x, np.float32)
    if x.ndim == 1:  # channel count is implicitly 1 (norm.rs:206)
        return ref.batch_norm(x.reshape(x.size, 1), scale, bias, mean, var, eps).reshape(x.shape)
    return ref.batch_norm(x, scale, bias, mean, var, eps)


def correctly_rounded_ln(s):
    return F(math.log(float(s)))


def exp_sum(row, mx):
    """sum of ReducedRangeExp(row - mx): acc[i % 16] += e_i in element order, then the 16 lanes added from lane 0."""
    exp = ref.lib().rto_exp_reduced_f32
    acc = [F(0)] * LANES
    d = (row - mx).astype(np.float32)
    for i in range(row.size):
        acc[i % LANES] = F(acc[i % LANES] + F(exp(float(d[i]))))
    s = F(0)
    for l in range(LANES):
        s = F(s + acc[l])
    return s


def log_softmax_row(row, ln=correctly_rounded_ln):
    row = np.asarray(row, np.float32)
    mx = F(np.finfo(np.float32).min)  # f32::MIN
    if row.size:
        mx = max(mx, row.max())
    s = exp_sum(row, mx)
    return ((row - mx).astype(np.float32) - F(ln(s))).astype(np.float32), s


def log_softmax(x, axis=-1, ln=correctly_rounded_ln):
    x = np.asarray(x, np.float32)
    t = np.ascontiguousarray(np.moveaxis(x, axis, -1))
    rows = t.reshape(-1, t.shape[-1]) if t.size else t.reshape(0, max(t.shape[-1], 1))
    y = np.empty_like(rows)
    with np.errstate(all="ignore"):
        for r in range(rows.shape[0]):
            y[r] = log_softmax_row(rows[r], ln)[0]
    return np.ascontiguousarray(np.moveaxis(y.reshape(t.shape), -1, axis))


def activation(kind, x, a=0.0, b=0.0):
    """The activation kinds as tests/test_gpu_activations.py computes its expectations: one rounded f32 operation at a time on the oracle's exp."""
    from rten_amd import lib as L
    x = np.asarray(x, np.float32)
    a, b = F(a), F(b)
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        def sigmoid(v):
            return one / (one + ref.exp(-v))

        def clamp01(v):
            v = np.where(v < zero, zero, v)
            return np.where(v > one, one, v).astype(np.float32)
        if kind == L.ACT_NONE:
            return x.copy()
        if kind == L.ACT_RELU:
            return ref.relu(x)
        if kind == L.ACT_GELU:
            return ref.gelu(x)
        if kind == L.ACT_SIGMOID:
            return sigmoid(x)
        if kind == L.ACT_SILU:
            return x / (one + ref.exp(-x))
        if kind == L.ACT_SWISH:
            return x * sigmoid(x * a)
        if kind == L.ACT_HARD_SIGMOID:
            return clamp01(a * x + b)
        if kind == L.ACT_HARD_SWISH:
            return x * clamp01((one / F(6)) * x + F(0.5))
        if kind == L.ACT_CLIP:
            y = np.where(x > a, x, a)
            return np.where(y < b, y, b).astype(np.float32)
        if kind == L.ACT_LEAKY_RELU:
            return np.where(x < zero, x * a, x).astype(np.float32)
        if kind == L.ACT_ELU:
            return np.where(x >= zero, x, a * (ref.exp(x) - one)).astype(np.float32)
    raise ValueError(kind)
