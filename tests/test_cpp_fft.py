"""Host side of DFT and STFT in the C++ layers: tests/cpp/test_fft_hostops.cpp checks attribute defaults and the opset-17 / opset-20 axis rule, what the loader refuses about the nodes by node name
without a device (the checks of rten_hip_run --parse-only), registry membership, the operators' own input checks and the reference's error strings,
batch coupling decided from the plan, and the host-only pass planner rten_hip_fft_plan.  Needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_fft_hostops")


def build_binary():
    from rten_amd import lib as L
    L.load()  # raises if librten_hip.so is missing: the C++ layer has no other backend
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_fft_hostops.cpp")
    deps = [src] + [os.path.join(ROOT, "include", h) for h in ("rten_hip_graph.hpp", "rten_hip_ops.hpp", "rten_hip.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", BIN, "-L" + os.path.join(ROOT, "rten_amd"),
                               "-lrten_hip", "-Wl,-rpath,$ORIGIN/../../../rten_amd", "-Wl,-rpath," + os.path.join(ROOT, "rten_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return BIN


def test_host_fft_operators_loader_refusals_and_planner():
    out = subprocess.run([build_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
