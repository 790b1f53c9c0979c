"""DFT and STFT on the device: rten_hip_dft_f32 / rten_hip_stft_f32 (rten_amd/csrc/fft.hip) against the EXACT transform and the error bound of
tests/fft_rules.py -- every specialised radix, generic passes, the direct pass, the LDS limit, lane counts around a workgroup's share, every loader and storer
rule, guarded and misaligned operands, NaN confinement -- then the Python operator, and onnx_writer.log_mel_graph / dft_graph / torch_export.log_mel_onnx
through the CLI (node by node, fused, unfused, captured), one loaded Graph at two batch sizes and two lengths, and the C-ABI model and its clone.

Every check prints `fft-ratio <what> <n_fft> <error / bound>`: the figures of docs/KERNELS.md 4.16."""
import os
import subprocess

import numpy as np
import pytest

from tests import confine as K
from tests import fft_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 12, 15, 16, 25, 30, 31, 37, 49, 64, 97, 100, 128, 400, 512, 1000, 1024, 4096, 8192]


def lanes_per_wg(n):
    """The kernel's rule: max(1, 256 r_max / n) whole lanes, at most 8192 points (rten_amd/csrc/fft.hip)."""
    from rten_amd import lib as L
    plan = L.fft_plan(n)
    return max(1, min(256 * max(plan + [1]) // n, L.FFT_MAX // n, 256))


def report(what, n, ratio):
    print(f"fft-ratio {what} {n} {ratio:.4f}")
    return ratio


def check_operand(g, arr, what):
    g.check(g.raw(), (arr.size,), (1,), F, what + " (an operand)")


def dft(ctx, x, n_fft, inverse=False, onesided=False, leads=(1, 2), what="", want=None):
    """The raw entry point on guarded input / output `lead` elements off a 16-byte boundary: x is [lanes, n_in, comp] -> the output, held to the bound."""
    lanes, n_in, comp = x.shape
    irfft, rfft = inverse and onesided, onesided and not inverse
    out_len, out_comp = (n_fft // 2 + 1 if rfft else n_fft), (1 if irfft else 2)
    xg, yg = K.Guarded(ctx, x if x.size else 4, lead=leads[0]), K.Guarded(ctx, max(lanes * out_len * out_comp, 1) * 4, lead=leads[1])
    ctx.call("rten_hip_dft_f32", lanes, n_in, n_fft, comp, 1 if inverse else 0, 1 if onesided else 0, xg.vp, yg.vp)
    what = f"dft {what} lanes {lanes} n_in {n_in} n_fft {n_fft} comp {comp} inverse {inverse} onesided {onesided} leads {leads}"
    shape = (lanes, out_len, out_comp)
    got = yg.check(yg.raw(), shape, K.dense(shape), F, what)
    if x.size:
        check_operand(xg, x, what)
    if want is None:
        want = R.dft(x, n_fft, -2, inverse, onesided)
    report("irfft" if irfft else "idft" if inverse else "rfft" if rfft else "dft", n_fft, R.assert_within_bound(got, want, n_fft, what=what))
    return got


def stft(ctx, signal, frame_step, window, n_fft, onesided=True, leads=(1, 2, 3), back=K.GUARD_FLAT, what=""):
    s3 = signal[..., None] if signal.ndim == 2 else signal
    batch, signal_len, comp = s3.shape
    n_frames, bins = (signal_len - n_fft) // frame_step + 1, (n_fft // 2 + 1 if onesided else n_fft)
    sg, yg = K.Guarded(ctx, signal, lead=leads[0], back=back), K.Guarded(ctx, batch * n_frames * bins * 8, lead=leads[2])
    wg = K.Guarded(ctx, window, lead=leads[1]) if window is not None else None
    ctx.call("rten_hip_stft_f32", batch, signal_len, comp, frame_step, n_fft, 1 if onesided else 0, wg.vp if wg else None, sg.vp, yg.vp)
    what = f"stft {what} batch {batch} len {signal_len} comp {comp} step {frame_step} n_fft {n_fft} window {window is not None} onesided {onesided} leads {leads}"
    shape = (batch, n_frames, bins, 2)
    got = yg.check(yg.raw(), shape, K.dense(shape), F, what)
    check_operand(sg, signal, what)
    if wg:
        check_operand(wg, window, what)
    want = R.stft(signal, frame_step, window, None if window is not None else n_fft, onesided)
    report("stft", n_fft, R.assert_within_bound(got, want, n_fft, what=what))
    return got


def noise(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


# ================================================================================================ the transform core
@pytest.mark.parametrize("n", LENGTHS)
def test_every_pass_kind_forward_and_inverse_real_and_complex(ctx, n):
    lanes = 3 if n < 4096 else 2
    for comp in (1, 2):
        x = noise(n + comp, lanes, n, comp)
        x[1] = 0  # a lane whose exact result is all zero comes out exactly zero
        for inverse in (False, True):
            got = dft(ctx, x, n, inverse=inverse)
            assert not got[1].any()
    dft(ctx, noise(n, lanes, n, 1), n, onesided=True)


def test_direct_pass_at_the_limit_and_the_refusal_above_it(ctx):
    from rten_amd import lib as L
    assert L.fft_plan(8191) == [8191]
    dft(ctx, noise(8191, 1, 8191, 2), 8191, what="one direct pass")
    x, y = K.Guarded(ctx, noise(1, 1, 8193, 1)), K.Guarded(ctx, 8193 * 8)
    with pytest.raises(L.HipError) as e:
        ctx.call("rten_hip_dft_f32", 1, 8193, 8193, 1, 0, 0, x.vp, y.vp)
    assert e.value.code == L.ERR_UNSUPPORTED and "8193" in str(e.value) and "8192" in str(e.value), str(e.value)
    with pytest.raises(L.HipError) as e:
        ctx.call("rten_hip_stft_f32", 1, 8193, 1, 1, 8193, 1, None, x.vp, y.vp)
    assert e.value.code == L.ERR_UNSUPPORTED and "8193" in str(e.value) and "8192" in str(e.value), str(e.value)
    y.check(y.raw(), (0,), (1,), F, "a refused call writes nothing")


@pytest.mark.parametrize("n", [16, 400])
def test_lane_counts_around_a_workgroup_s_share(ctx, n):
    lpw = lanes_per_wg(n)
    assert lpw == {16: 64, 400: 3}[n]
    for lanes in sorted({1, lpw - 1, lpw, lpw + 1}):
        dft(ctx, noise(lanes, lanes, n, 2), n, what="lane count")
        dft(ctx, noise(lanes, lanes, n, 1), n, onesided=True, what="lane count")


@pytest.mark.parametrize("n", [8, 9, 400, 25])
def test_irfft_rebuilds_the_conjugate_half(ctx, n):
    half = n // 2 + 1
    for n_in in sorted({1, half - 1, half, half + 1, n, n + 3}):
        x = noise(n + n_in, 3, n_in, 2)
        dft(ctx, x, n, inverse=True, onesided=True, what=f"n_in {n_in} against N/2+1 = {half}")
    # a half spectrum of a real signal comes back as that signal
    sig = noise(n, 2, n, 1)
    spec = dft(ctx, sig, n, onesided=True)
    back = dft(ctx, spec, n, inverse=True, onesided=True)
    c = R.EPS * 2 * R.bound_constant(n)
    assert np.sqrt(((back - sig).astype(np.float64) ** 2).sum()) <= c * np.sqrt((sig.astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("n_in,n_fft", [(5, 12), (12, 5), (1, 16), (100, 37), (37, 100), (401, 400)])
def test_zero_fill_and_truncation(ctx, n_in, n_fft):
    for comp in (1, 2):
        dft(ctx, noise(n_in, 3, n_in, comp), n_fft, what="zero-fill / truncate")
        dft(ctx, noise(n_in, 3, n_in, comp), n_fft, inverse=True, what="zero-fill / truncate")
    dft(ctx, noise(n_in, 3, n_in, 1), n_fft, onesided=True, what="zero-fill / truncate")


def test_empty_transforms(ctx):
    got = dft(ctx, np.zeros((3, 0, 1), F), 0, onesided=True, what="n_fft == 0 one-sided: one zero bin", want=np.zeros((3, 1, 2)))
    assert got.shape == (3, 1, 2) and not got.any()
    y = K.Guarded(ctx, 64)
    ctx.call("rten_hip_dft_f32", 0, 4, 4, 1, 0, 0, None, y.vp)
    ctx.call("rten_hip_dft_f32", 3, 0, 0, 2, 0, 0, None, y.vp)
    ctx.call("rten_hip_stft_f32", 0, 8, 1, 2, 4, 1, None, None, y.vp)
    y.check(y.raw(), (0,), (1,), F, "empty calls write nothing")


@pytest.mark.parametrize("n", [12, 37, 400, 1024])
def test_forward_then_inverse_returns_the_input(ctx, n):
    x = noise(n, 4, n, 2)
    spec = dft(ctx, x, n)
    back = dft(ctx, spec, n, inverse=True)
    err = np.sqrt(((back - x).astype(np.float64) ** 2).sum(axis=(1, 2)))
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=(1, 2)))
    ratio = float((err / (R.EPS * 2 * R.bound_constant(n) * norm)).max())  # the sum of the two bounds
    report("round-trip", n, ratio)
    assert ratio <= 1.0


def test_a_nan_stays_in_its_lane(ctx):
    for n in (16, 400, 37):
        x = noise(n, 2 * lanes_per_wg(n) + 1, n, 2)
        clean = dft(ctx, x, n)
        bad = x.copy()
        hit = lanes_per_wg(n) // 2
        bad[hit, n // 3, 0] = np.nan
        lanes, n_in, comp = bad.shape
        xg, yg = K.Guarded(ctx, bad), K.Guarded(ctx, clean.nbytes)
        ctx.call("rten_hip_dft_f32", lanes, n_in, n, comp, 0, 0, xg.vp, yg.vp)
        got = yg.check(yg.raw(), clean.shape, K.dense(clean.shape), F, "nan lane")
        others = np.arange(lanes) != hit
        assert np.array_equal(got[others].view(np.uint32), clean[others].view(np.uint32)), n  # every other lane: the same bits
        assert np.isnan(got[hit]).any(), n  # (a NaN real part leaves what only the imaginary parts feed: exact zeros and +-i rotations multiply nothing)


# ================================================================================================ STFT
@pytest.mark.parametrize("step", [1, 16, 23])
@pytest.mark.parametrize("form", ["window", "frame_length"])
def test_stft_steps_and_forms(ctx, step, form):
    n = 16
    window = (np.hanning(n + 1)[:n]).astype(F) if form == "window" else None
    stft(ctx, noise(step, 2, 75), step, window, n, what="2-D signal")
    stft(ctx, noise(step, 2, 75, 1), step, window, n, onesided=False, what="3-D real, two-sided")
    stft(ctx, noise(step, 2, 75, 2), step, window, n, onesided=False, what="complex")


@pytest.mark.parametrize("n,step,length", [(400, 160, 1400), (37, 10, 120), (12, 5, 12), (400, 400, 400)])
def test_stft_frames(ctx, n, step, length):
    window = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(F)
    got = stft(ctx, noise(n, 3, length), step, window, n, what="frames")
    assert got.shape[1] == (length - n) // step + 1 and (length != n or got.shape[1] == 1)


@pytest.mark.parametrize("leads", [(0, 0, 0), (1, 2, 3), (3, 1, 2), (2, 3, 1)])
def test_stft_tail_shorter_than_a_step_is_never_read(ctx, leads):
    """The last frame ends on the LAST element of the allocation (no back guard at all): the 3 samples behind it that a fourth frame would need do not exist."""
    n, step = 16, 7
    signal = noise(5, 1, n + 2 * step)  # 3 frames, the last ends at the end; a tail of 0
    stft(ctx, signal, step, None, n, leads=leads, back=0, what="last frame at the end of the allocation")
    longer = noise(6, 1, n + 2 * step + 3)  # a tail of 3 < step: covered by no frame
    got = stft(ctx, longer, step, None, n, leads=leads, back=0, what="tail")
    poisoned = longer.copy()
    poisoned[0, -3:] = np.nan
    sg, yg = K.Guarded(ctx, poisoned, lead=leads[0], back=0), K.Guarded(ctx, got.nbytes, lead=leads[2])
    ctx.call("rten_hip_stft_f32", 1, poisoned.shape[1], 1, step, n, 1, None, sg.vp, yg.vp)
    again = yg.check(yg.raw(), got.shape, K.dense(got.shape), F, "tail of NaNs")
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_a_nan_sample_reaches_exactly_the_frames_that_cover_it(ctx):
    n, step = 16, 5
    signal = noise(9, 2, 90)
    clean = stft(ctx, signal, step, None, n)
    bad = signal.copy()
    at = 41
    bad[1, at] = np.nan
    sg, yg = K.Guarded(ctx, bad), K.Guarded(ctx, clean.nbytes)
    ctx.call("rten_hip_stft_f32", 2, 90, 1, step, n, 1, None, sg.vp, yg.vp)
    got = yg.check(yg.raw(), clean.shape, K.dense(clean.shape), F, "nan sample")
    frames = np.arange(clean.shape[1])
    covered = (frames * step <= at) & (at < frames * step + n)
    assert covered.sum() == 3
    assert np.isnan(got[1, covered]).any(axis=(1, 2)).all()
    assert np.array_equal(got[1, ~covered].view(np.uint32), clean[1, ~covered].view(np.uint32)) and np.array_equal(got[0].view(np.uint32), clean[0].view(np.uint32))


# ================================================================================================ the Python operator
def test_python_operators_on_the_device(ctx):
    import json
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    dev = lambda a: DeviceTensor.from_numpy(ctx, np.ascontiguousarray(a, F))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "fft_reference.json")))
    for case in golden["dft"]:
        x = np.asarray(case["input"], F).reshape(case.get("input_shape", np.asarray(case["input"]).shape))
        inputs = [dev(x), None if case["dft_length"] is None else np.array(case["dft_length"], np.int64), np.array(case["axis"], np.int64)]
        op = ops.DFT(case["inverse"], case["onesided"])
        if "error" in case:
            with pytest.raises(ops.OpError) as e:
                op.run(ctx, inputs)
            assert [e.value.kind, e.value.msg] == case["error"], case["name"]
            continue
        y = op.run(ctx, inputs)[0].numpy()
        want = np.asarray(case["expected"], F).reshape(case.get("expected_shape", np.asarray(case["expected"]).shape))
        assert y.shape == want.shape and np.abs(y - want).max() <= golden["tolerance"], case["name"]
    for case in golden["stft"]:
        inputs = [dev(case["signal"]), np.array(case["frame_step"], np.int64), None if case["window"] is None else dev(case["window"]),
                  None if case["frame_length"] is None else np.array(case["frame_length"], np.int64)]
        op = ops.STFT(case["onesided"])
        if "error" in case:
            with pytest.raises(ops.OpError) as e:
                op.run(ctx, inputs)
            assert [e.value.kind, e.value.msg] == case["error"], case["name"]
            continue
        y = op.run(ctx, inputs)[0].numpy()
        want = np.asarray(case["expected"], F)
        assert y.shape == want.shape and np.abs(y - want).max() <= golden["tolerance"], case["name"]


@pytest.mark.parametrize("shape,axis", [((5, 2), 0), ((3, 12, 2), -2), ((1, 4, 2, 1), 1), ((6, 3, 5, 2), 0), ((2, 7, 3, 1), -3), ((2, 3, 8, 2), -4)])
def test_python_dft_axes(ctx, shape, axis):
    from rten_amd import ops
    from rten_amd.tensor import DeviceTensor
    x = noise(sum(shape), *shape)
    nd = len(shape)
    ax = axis + nd if axis < 0 else axis
    for inverse, onesided, length in ((False, False, None), (True, False, None), (False, shape[-1] == 1, shape[ax] + 2), (shape[-1] == 2, shape[-1] == 2, None)):
        inputs = [DeviceTensor.from_numpy(ctx, x), None if length is None else np.array([length], np.int64), np.array(axis, np.int64)]
        y = ops.DFT(inverse, onesided).run(ctx, inputs)[0].numpy()
        want = R.dft(x, length, axis, inverse, onesided)
        n_fft = length if length is not None else (2 * (shape[ax] - 1) if inverse and onesided else shape[ax])
        assert y.shape == want.shape, (y.shape, want.shape)
        if n_fft:
            report("axis", n_fft, R.assert_within_bound(y, want, n_fft, lane_axis=ax, what=f"DFT {shape} axis {axis} inverse {inverse} onesided {onesided}"))
    assert ops.DFT().batch_coupled(shape, axis) == (ax == 0)


# ================================================================================================ graphs
from tests.test_gpu_sample import SESSION_TIMEOUT_S, run_cli_graph  # noqa: E402

CLI_MODES = [("-t",), (), ("--no-fuse",), ("--graph",)]


def log_mel_f64(wave, n_fft, hop, window, mel):
    """float64 NumPy evaluation of the log-mel module from the float32 wave, window and filterbank -> (spectrum [b, f, bins, 2], log_mel [b, f, mels])."""
    pad = n_fft // 2
    padded = np.pad(wave, ((0, 0), (pad, pad)), mode="reflect")
    frames = (padded.shape[1] - n_fft) // hop + 1
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    z = padded[:, idx].astype(np.float64) * window.astype(np.float64)
    spec = np.fft.rfft(z, axis=-1)
    power = spec.real ** 2 + spec.imag ** 2
    l = np.log10(np.maximum(power @ mel.astype(np.float64), 1e-10))
    l = np.maximum(l, l.max() - 8.0)
    return np.stack([spec.real, spec.imag], -1), (l + 4.0) / 4.0


def log_mel_torch_f32(wave, n_fft, hop, window, mel):
    """PyTorch's own float32 CPU forward of the same module."""
    import torch
    s = torch.stft(torch.from_numpy(wave), n_fft, hop, window=torch.from_numpy(window), center=True, pad_mode="reflect", return_complex=True)
    power = (s.real ** 2 + s.imag ** 2).transpose(1, 2)
    l = torch.clamp(power @ torch.from_numpy(mel), min=1e-10).log10()
    l = torch.maximum(l, l.max() - 8.0)
    return ((l + 4.0) / 4.0).numpy()


def check_log_mel(got, wave, n_fft, hop, w, what):
    """spectrum to the FFT bound (against the exact STFT of the float32 window * signal products); log_mel within 4x PyTorch's own float32 error."""
    spec64, want = log_mel_f64(wave, n_fft, hop, w["window"], w["mel"])
    pad = n_fft // 2
    if "spectrum" in got:
        exact = R.stft(np.pad(wave, ((0, 0), (pad, pad)), mode="reflect"), hop, w["window"], None, True)
        report("graph-stft", n_fft, R.assert_within_bound(got["spectrum"].reshape(exact.shape), exact, n_fft, what=what + " (the STFT node's output)"))
    torch_err = float(np.abs(log_mel_torch_f32(wave, n_fft, hop, w["window"], w["mel"]) - want).max())
    ours = float(np.abs(got["log_mel"].reshape(want.shape) - want).max())
    print(f"fft-logmel {what}: max abs error {ours:.3e}, PyTorch f32 CPU {torch_err:.3e}, allowance {4 * torch_err:.3e}")
    assert ours <= 4 * torch_err, (what, ours, torch_err)


LM = dict(n_fft=400, hop=160, n_mels=20)


@pytest.mark.parametrize("extra", CLI_MODES, ids=["node by node", "fused", "unfused", "captured"])
def test_log_mel_graph_through_the_cli(ctx, tmp_path, extra):
    from rten_amd import onnx_writer as ow
    data, w = ow.log_mel_graph(expose_stft=True, **LM)
    wave = noise(17, 2, 2000)
    got, log = run_cli_graph(tmp_path, data, {"wave": wave}, ["log_mel", "spectrum"], {"batch": 2, "samples": 2000}, extra)
    check_log_mel(got, wave, LM["n_fft"], LM["hop"], w, f"log_mel_graph cli {extra}")
    if extra == ("-t",):
        assert "STFT" in log
    if extra == ("--graph",):
        assert "Captured" in log, log[-1500:]


def dft_graph_want(x, w, dft_length):
    spec = R.dft(x, dft_length, 1, False, False)
    filtered = (spec.astype(F) * w["gain"]).astype(F)  # (the graph's own f32 spectrum is within the bound of this one; the check below allows for both passes)
    return spec, R.dft(filtered, None, 1, True, False)


@pytest.mark.parametrize("opset,n,length", [(17, 12, None), (20, 12, None), (20, 30, 37), (17, 100, 64)])
def test_dft_graph_through_the_cli(ctx, tmp_path, opset, n, length):
    from rten_amd import onnx_writer as ow
    data, w = ow.dft_graph(opset=opset, n=n, dft_length=length)
    n_fft = length or n
    x = noise(opset + n, 3, n, 1)
    for extra in CLI_MODES:
        got, log = run_cli_graph(tmp_path, data, {"x": x}, ["y", "spectrum"], {"batch": 3}, extra)
        spec = got["spectrum"].reshape(3, n_fft, 2)
        report("graph-dft", n_fft, R.assert_within_bound(spec, R.dft(x, length, 1, False, False), n_fft, lane_axis=1, what=f"dft_graph opset {opset} {extra} forward"))
        filtered = (spec * w["gain"]).astype(F)  # the product the graph formed, from the spectrum the SAME run produced
        report("graph-idft", n_fft, R.assert_within_bound(got["y"].reshape(3, n_fft, 2), R.dft(filtered, None, 1, True, False), n_fft, lane_axis=1,
                                                          what=f"dft_graph opset {opset} {extra} inverse"))


def session(tmp_path, data, script_of):
    """ONE loaded Graph in one process of tests/cpp/graph_session.cpp running `script_of(dir)` = [(line words, output path or None)] -> {path: {name: array}}."""
    from tests import graph_sessions as gs
    from tests.test_gpu_graph_fuzz import read_safetensors
    d = str(tmp_path)
    open(os.path.join(d, "session.onnx"), "wb").write(data)
    lines = script_of(d)
    open(os.path.join(d, "script.txt"), "w").write("\n".join(" ".join(words) for words, _ in lines) + "\n")
    r = subprocess.run([gs.build_session_probe(), os.path.join(d, "session.onnx"), os.path.join(d, "script.txt")], capture_output=True, text=True, timeout=SESSION_TIMEOUT_S)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return [dict(read_safetensors(out)) for _, out in lines if out]


def test_one_loaded_log_mel_model_at_two_batch_sizes_and_two_lengths(ctx, tmp_path):
    from safetensors.numpy import save_file
    from rten_amd import onnx_writer as ow
    data, w = ow.log_mel_graph(expose_stft=True, **LM)
    waves = [noise(31, 1, 1600), noise(32, 3, 2333), noise(33, 1, 1600), noise(34, 3, 1600)]

    def script(d):
        lines = []
        for k, wave in enumerate(waves):
            save_file({"wave": wave}, os.path.join(d, f"b{k}.safetensors"))
            lines.append((["run", os.path.join(d, f"b{k}.safetensors"), os.path.join(d, f"out{k}.safetensors")], os.path.join(d, f"out{k}.safetensors")))
        lines.append((["capture", os.path.join(d, "b1.safetensors"), os.path.join(d, "cap.safetensors")], os.path.join(d, "cap.safetensors")))
        lines.append((["replay", os.path.join(d, "rep.safetensors")], os.path.join(d, "rep.safetensors")))
        lines.append((["run", os.path.join(d, "b0.safetensors"), os.path.join(d, "again.safetensors")], os.path.join(d, "again.safetensors")))
        return lines

    outs = session(tmp_path, data, script)
    for k, (got, wave) in enumerate(zip(outs, waves + [waves[1], waves[1], waves[0]])):
        check_log_mel({nm: a.view(F) for nm, a in got.items()}, wave, LM["n_fft"], LM["hop"], w, f"one graph, step {k}")
    assert np.array_equal(outs[4]["log_mel"].view(np.uint32), outs[5]["log_mel"].view(np.uint32))  # the replay is the captured run again
    assert np.array_equal(outs[0]["log_mel"].view(np.uint32), outs[6]["log_mel"].view(np.uint32))  # the kernels are deterministic


def model_outputs(ctx, m, feeds):
    from rten_amd.tensor import DeviceTensor
    for name in m.inputs:
        a = feeds[name]
        DeviceTensor(ctx, a.shape, a.dtype, ptr=m.bind_input(name, a.shape), keepalive=m).upload(a)
    ctx.sync()
    m.prepare()  # captures
    m.run()
    m.sync()
    out = {}
    for i, name in enumerate(m.outputs):
        ptr, shape = m.output(i)
        out[name] = DeviceTensor(ctx, shape, F, ptr=ptr, keepalive=m).numpy()
    return out


def test_c_abi_model_captures_the_front_end_and_so_does_its_clone(ctx):
    from rten_amd import lib as L
    from rten_amd import onnx_writer as ow
    data, w = ow.log_mel_graph(expose_stft=True, **LM)
    m, other = L.Model(ctx, data), L.Context(0)
    try:
        wave = noise(51, 2, 1800)
        check_log_mel(model_outputs(ctx, m, {"wave": wave}), wave, LM["n_fft"], LM["hop"], w, "the C-ABI model, captured")
        lane = m.clone(other)
        try:
            wave = noise(52, 2, 1800)
            check_log_mel(model_outputs(other, lane, {"wave": wave}), wave, LM["n_fft"], LM["hop"], w, "its clone on a second context")
        finally:
            lane.close()
    finally:
        m.close()
        other.close()


def test_exported_torch_module_runs_from_the_waveform(ctx, tmp_path):
    """torch.stft -> power -> mel -> log10 -> floor -> affine through PyTorch's exporter (tools/torch_export.log_mel_onnx): the graph the issue names."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch_export
    data, w = torch_export.log_mel_onnx(n_fft=LM["n_fft"], hop=LM["hop"], n_mels=LM["n_mels"])
    wave = noise(61, 3, 2100)  # (neither the batch size nor the length the exporter traced)
    for extra in ((), ("--no-fuse",), ("--graph",)):
        got, log = run_cli_graph(tmp_path, data, {"wave": wave}, ["log_mel"], {"batch": 3, "samples": 2100}, extra)
        check_log_mel(got, wave, LM["n_fft"], LM["hop"], w, f"torch export {extra}")


def test_host_layer_errors_carry_the_reference_s_strings(ctx, tmp_path):
    """The C++ host layer, through the CLI: a transform above the limit is refused with the entry point's words."""
    from rten_amd import onnx_writer as ow
    from tests.test_graph_executor import run_cli
    path = tmp_path / "model.onnx"
    data, _ = ow.dft_graph(opset=20, n=8, dft_length=8193)
    path.write_bytes(data)
    r = run_cli("-s", "batch=1", str(path))
    assert r.returncode != 0 and "DFT transform of length 8193 exceeds the limit of 8192 points" in r.stdout + r.stderr, r.stdout[-1500:] + r.stderr[-1500:]
