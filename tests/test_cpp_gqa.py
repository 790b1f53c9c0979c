"""Host side of com.microsoft GroupQueryAttention in the C++ layers: tests/cpp/test_gqa_hostops.cpp checks attribute defaults, the registry name, what the loader
reads and refuses about the node by node name without a device (the checks of rten_hip_run --parse-only), the operator's own input checks with the reference's
error strings, and the plan a graph with the node compiles to (one step, nothing read back, not batch-coupled).  Built twice: -Wall -Werror, and as a stand-alone
program under -fsanitize=address,undefined.  Needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_gqa_hostops")


def build_binary(sanitize=False):
    from rten_amd import lib as L
    L.load()  # raises if librten_hip.so is missing: the C++ layer has no other backend
    out = BIN + ("_asan" if sanitize else "")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_gqa_hostops.cpp")
    deps = [src] + [os.path.join(ROOT, "include", h) for h in ("rten_hip_graph.hpp", "rten_hip_ops.hpp", "rten_hip.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        # (the sanitizer runtimes linked statically, as tests/graph_sessions.py links its probe: the program runs whatever else the environment loads first)
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] if sanitize else ["-O1"]
        subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", out, "-L" + os.path.join(ROOT, "rten_amd"),
                               "-lrten_hip", "-Wl,-rpath,$ORIGIN/../../../rten_amd", "-Wl,-rpath," + os.path.join(ROOT, "rten_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_host_gqa_operator_loader_refusals_and_plan():
    out = subprocess.run([build_binary()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_the_same_program_is_clean_under_address_and_undefined_behaviour_sanitizers():
    out = subprocess.run([build_binary(sanitize=True)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
