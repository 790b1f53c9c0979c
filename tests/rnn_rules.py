"""GRU and LSTM as the reference computes them (src/ops/rnn.rs:138-328, 413-597), restated in numpy one rounded f32 operation at a time
on top of the oracle's GEMM, exp and tanh.  The expected value of every recurrent-layer test.

    GRU   gates = x_t.W^T (+ Wb); hs = h.R^T (+ Rb); z, r = sigmoid(gates[z|r] + hs[z|r]); g = tanh(gates[h] + hs[h] * r);
          h = (1 - z) * g + z * h                                  gate order update, reset, hidden
    LSTM  gates = x_t.W^T (+ Wb); gates = 1 * gates + h.R^T (GEMM with beta = 1 into the same buffer); (+ Rb); i, o, f = sigmoid, g = tanh;
          c = f * c + i * g; h = o * tanh(c)                       gate order input, output, forget, cell

Below PREPACK_MIN_SEQ_LEN = 5 time steps the reference's weights are unpacked, and a one-row product of unpacked operands takes its
vector-matrix kernels (rten-gemm/src/lib.rs:876): `ref.gemm_f32` makes that choice for M == 1 while `ref.set_gemv_enabled` is on, so the
restatement switches it off for every product of a layer with 5 or more steps.

`cell_tanh` is the function in h = o * tanh(c): the reference calls Rust's f32::tanh (the host's libm) there; the backend uses the vecmath tanh
(docs/KERNELS.md), and so does the default here.
"""
import numpy as np

from oracle import ref

PREPACK_MIN_SEQ_LEN = 5
DIRECTIONS = ("forward", "reverse", "bidirectional")

_ONE = np.float32(1.0)


def sigmoid(x):
    """1 / (1 + exp(-x)) on the vecmath exp (rten-vecmath/src/exp.rs:201-230)."""
    x = np.asarray(x, np.float32)
    return (_ONE / (_ONE + ref.exp(-x))).astype(np.float32)


def _steps(direction, d, seq):
    rev = (direction == "reverse" and d == 0) or (direction == "bidirectional" and d == 1)
    return range(seq - 1, -1, -1) if rev else range(seq)


def _dirs(direction):
    assert direction in DIRECTIONS, direction
    return 2 if direction == "bidirectional" else 1


class _Products:
    """The reference's choice between its packed (blocked) and unpacked (one-row capable) products for one layer."""

    def __init__(self, seq):
        self.blocked_only = seq >= PREPACK_MIN_SEQ_LEN

    def __enter__(self):
        if self.blocked_only:
            ref.set_gemv_enabled(False)
        return self

    def __exit__(self, *exc):
        ref.set_gemv_enabled(True)


def gru(x, w, r, b=None, h0=None, direction="forward"):
    """-> (Y [seq, dirs, batch, hidden], Y_h [dirs, batch, hidden])"""
    x, w, r = (np.ascontiguousarray(a, np.float32) for a in (x, w, r))
    seq, batch, _ = x.shape
    dirs, H = _dirs(direction), w.shape[1] // 3
    h = np.zeros((dirs, batch, H), np.float32) if h0 is None else np.array(h0, np.float32)
    y = np.zeros((seq, dirs, batch, H), np.float32)
    with _Products(seq):
        for d in range(dirs):
            wt, rt = w[d].T, r[d].T
            for t in _steps(direction, d, seq):
                gates = ref.gemm_f32(x[t], wt)
                if b is not None:
                    gates = gates + b[d, :3 * H].astype(np.float32)
                hs = ref.gemm_f32(h[d], rt)
                if b is not None:
                    hs = hs + b[d, 3 * H:].astype(np.float32)
                zr = sigmoid(gates[:, :2 * H] + hs[:, :2 * H])
                z, rg = zr[:, :H], zr[:, H:]
                hh = hs[:, 2 * H:] * rg
                g = ref.tanh(gates[:, 2 * H:] + hh)
                h[d] = ((_ONE - z) * g).astype(np.float32) + (z * h[d]).astype(np.float32)
                y[t, d] = h[d]
    return y, h


def lstm(x, w, r, b=None, h0=None, c0=None, direction="forward", cell_tanh=None):
    """-> (Y, Y_h, Y_c)"""
    cell_tanh = cell_tanh or ref.tanh
    x, w, r = (np.ascontiguousarray(a, np.float32) for a in (x, w, r))
    seq, batch, _ = x.shape
    dirs, H = _dirs(direction), w.shape[1] // 4
    h = np.zeros((dirs, batch, H), np.float32) if h0 is None else np.array(h0, np.float32)
    c = np.zeros((dirs, batch, H), np.float32) if c0 is None else np.array(c0, np.float32)
    y = np.zeros((seq, dirs, batch, H), np.float32)
    with _Products(seq):
        for d in range(dirs):
            wt, rt = w[d].T, r[d].T
            for t in _steps(direction, d, seq):
                gates = ref.gemm_f32(x[t], wt)
                if b is not None:
                    gates = gates + b[d, :4 * H].astype(np.float32)
                gates = ref.gemm_f32(h[d], rt, c=gates, beta=1.0)
                if b is not None:
                    gates = gates + b[d, 4 * H:].astype(np.float32)
                iof = sigmoid(gates[:, :3 * H])
                ig, og, fg = iof[:, :H], iof[:, H:2 * H], iof[:, 2 * H:]
                cg = ref.tanh(gates[:, 3 * H:])
                c[d] = (fg * c[d]).astype(np.float32) + (ig * cg).astype(np.float32)
                h[d] = og * np.asarray(cell_tanh(c[d]), np.float32)
                y[t, d] = h[d]
    return y, h, c


def lstm_f64(x, w, r, b=None, h0=None, c0=None, direction="forward"):
    """The same layer in float64 with numpy's functions: the yardstick of the tanh-divergence bound."""
    x, w, r = (np.asarray(a, np.float64) for a in (x, w, r))
    seq, batch, _ = x.shape
    dirs, H = _dirs(direction), w.shape[1] // 4
    h = np.zeros((dirs, batch, H)) if h0 is None else np.array(h0, np.float64)
    c = np.zeros((dirs, batch, H)) if c0 is None else np.array(c0, np.float64)
    y = np.zeros((seq, dirs, batch, H))
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))
    for d in range(dirs):
        for t in _steps(direction, d, seq):
            gates = x[t] @ w[d].T + h[d] @ r[d].T
            if b is not None:
                gates = gates + np.asarray(b[d, :4 * H], np.float64) + np.asarray(b[d, 4 * H:], np.float64)
            ig, og, fg = sg(gates[:, :H]), sg(gates[:, H:2 * H]), sg(gates[:, 2 * H:3 * H])
            c[d] = fg * c[d] + ig * np.tanh(gates[:, 3 * H:])
            h[d] = og * np.tanh(c[d])
            y[t, d] = h[d]
    return y, h, c


def reorder_gates(a, src, dst, axis):
    """PyTorch's gate blocks along `axis` in the reference's order, as its own test does (rnn.rs:870-1011): "ifco" -> "iofc", "ruh" -> "urh"."""
    parts = np.split(np.asarray(a), len(src), axis=axis)
    return np.concatenate([parts[src.index(g)] for g in dst], axis=axis)
