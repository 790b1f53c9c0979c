"""The yardstick of DFT and STFT: the EXACT transform of the float32 inputs, in NumPy float64, and the error bound the kernels are held to.

The reference computes these operators with an FFT library, so the contract is not bit-identity but a bound against the exact result.  Everything here
follows the reference's rules (src/ops/fft.rs) on float64 data: the lane is truncated or zero-filled to n_fft, IRFFT rebuilds the conjugate half exactly as
the reference does (for even n_fft the Nyquist bin is left as given; bins at k >= n_in are zero), the inverse's scale is the float32 value 1.0f / n_fft
applied as a float64 multiply, and STFT forms window * signal in float32 first (one rounded multiply, as the reference does) and widens the product.

The bound, per lane (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2, generalised from radix 2: a pass of radix r sums r products with
twiddles that carry at most eps / 2 error, relative 2-norm error (2 r + 6) eps to first order):

    ||got - want||_2 <= eps_f32 * C(n) * ||want||_2,    C(n) = 2 + sum over the passes of rten_hip_fft_plan(n) of (2 r + 6)

with the passes read from the library's own plan (rten_amd.lib.fft_plan), never from a copy of the factoring.  A lane whose exact result is all zero must
come out exactly zero."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)


def bound_constant(n):
    from rten_amd import lib
    return 2.0 + sum(2.0 * r + 6.0 for r in lib.fft_plan(n)) if n >= 1 else 2.0


def _resolve_axis(nd, axis):
    if axis < -nd or axis >= nd:
        raise ValueError("Axis is invalid")
    return axis + nd if axis < 0 else axis


def dft_error(shape, dft_length, axis, inverse, onesided):
    """The reference's refusal of a DFT call, as its message, or None (fft.rs:208-258, in its order)."""
    nd = len(shape)
    if nd < 2:
        return "DFT input must have at least 2 dims"
    if shape[-1] not in (1, 2):
        return "Last dimension of DFT input must have size 1 or 2"
    if inverse and onesided and shape[-1] != 2:
        return "Inverse one-sided DFT (IRFFT) requires complex input"
    if onesided and not inverse and shape[-1] == 2:
        return "DFT cannot be one-sided if input is complex"
    if not -nd <= axis < nd:
        return "Axis is invalid"
    if _resolve_axis(nd, axis) == nd - 1:
        return "DFT axis cannot be the complex dimension"
    if dft_length is not None and dft_length < 1:
        return "dft_length must be >= 1"
    return None


def dft(x, dft_length=None, axis=-2, inverse=False, onesided=False):
    """The exact DFT of float32 `x` [..., n, 1 | 2] along `axis`, float64, in the input's axis order."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    err = dft_error(x.shape, dft_length, axis, inverse, onesided)
    if err:
        raise ValueError(err)
    nd = x.ndim
    ax = _resolve_axis(nd, axis)
    irfft = inverse and onesided
    signal_len = x.shape[ax]
    n_fft = dft_length if dft_length is not None else (2 * max(signal_len - 1, 0) if irfft else signal_len)
    out_len = n_fft // 2 + 1 if onesided and not inverse else n_fft
    z = np.moveaxis(x.astype(np.float64), ax, -2)
    z = z[..., 0] + 1j * z[..., 1] if x.shape[-1] == 2 else z[..., 0] + 0j  # [..., signal_len]
    n_in = min(signal_len, n_fft)
    buf = np.zeros(z.shape[:-1] + (n_fft,), np.complex128)
    buf[..., :n_in] = z[..., :n_in]
    if irfft:
        conj_end = max(n_in - 1, 0) if n_fft % 2 == 0 else n_in
        for k in range(1, conj_end):
            buf[..., n_fft - k] = np.conj(z[..., k])
    if n_fft == 0:
        spec = np.zeros(z.shape[:-1] + (out_len,), np.complex128)
    elif inverse:
        spec = np.fft.ifft(buf, axis=-1) * n_fft * float(np.float32(1.0) / np.float32(n_fft))
    else:
        spec = np.fft.fft(buf, axis=-1)
    spec = spec[..., :out_len]
    out = spec.real[..., None] if irfft else np.stack([spec.real, spec.imag], axis=-1)
    return np.moveaxis(out, -2, ax)


def stft_error(shape, frame_step, window_len, frame_length, onesided):
    """The reference's refusal of an STFT call, as its message, or None (fft.rs:30-93, in its order); window_len None = no window."""
    if len(shape) not in (2, 3):
        return "signal must have 2 or 3 dims"
    signal_len = shape[1]
    if frame_length is not None and not 1 <= frame_length <= signal_len:
        return "frame_length must be in range [1, signal_length]"
    if frame_step <= 0:
        return "frame_step must be > 0"
    if frame_length is not None and window_len is not None and frame_length != window_len:
        return "window length must equal frame_length"
    if frame_length is None and window_len is None:
        return "Either frame_length or window must be set"
    comp = shape[2] if len(shape) == 3 else 1
    if comp not in (1, 2):
        return "Last dimension of signal must have size 1 or 2"
    if comp == 2 and onesided:
        return "FFT cannot be one-sided if input is complex"
    return None


def stft(signal, frame_step, window=None, frame_length=None, onesided=True):
    """The exact STFT of float32 `signal` [batch, len] or [batch, len, 1 | 2]: float64 [batch, n_frames, bins, 2]."""
    signal = np.asarray(signal)
    assert signal.dtype == np.float32 and (window is None or np.asarray(window).dtype == np.float32)
    err = stft_error(signal.shape, frame_step, None if window is None else len(window), frame_length, onesided)
    if err:
        raise ValueError(err)
    s = signal[..., None] if signal.ndim == 2 else signal
    batch, signal_len, comp = s.shape
    n_fft = frame_length if frame_length is not None else len(window)
    n_frames = (signal_len - n_fft) // frame_step + 1
    bins = n_fft // 2 + 1 if onesided else n_fft
    idx = np.arange(n_frames)[:, None] * frame_step + np.arange(n_fft)[None, :]
    frames = s[:, idx, :]  # [batch, n_frames, n_fft, comp], float32
    if window is not None:
        frames = np.asarray(window, np.float32)[None, None, :, None] * frames  # ONE rounded float32 multiply
        assert frames.dtype == np.float32
    z = frames.astype(np.float64)
    z = z[..., 0] + 1j * z[..., 1] if comp == 2 else z[..., 0] + 0j
    spec = np.fft.fft(z, axis=-1)[..., :bins]
    return np.stack([spec.real, spec.imag], axis=-1)


def lane_ratios(got, want, n_fft, lane_axis=-2):
    """error / bound of every lane: `got` (float32) and `want` (float64) hold lanes along `lane_axis` (the component axis is last).  A lane whose exact
    result is all zero must be exactly zero: its ratio is 0 then, inf otherwise."""
    got = np.moveaxis(np.asarray(got, np.float64), lane_axis, -2)
    want = np.moveaxis(np.asarray(want, np.float64), lane_axis, -2)
    assert got.shape == want.shape, (got.shape, want.shape)
    g = got.reshape(-1, got.shape[-2] * got.shape[-1])
    w = want.reshape(g.shape)
    err = np.sqrt(((g - w) ** 2).sum(axis=1))
    norm = np.sqrt((w ** 2).sum(axis=1))
    bound = EPS * bound_constant(n_fft) * norm
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(norm == 0, np.where(err == 0, 0.0, np.inf), err / bound)
    return r


def assert_within_bound(got, want, n_fft, lane_axis=-2, what=""):
    r = lane_ratios(got, want, n_fft, lane_axis)
    worst = float(r.max()) if r.size else 0.0
    assert np.all(np.isfinite(np.asarray(got))) or not np.all(np.isfinite(want)), f"{what}: non-finite output"
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3g} at lane {int(r.argmax())} (n_fft {n_fft}, C = {bound_constant(n_fft)})"
    return worst
