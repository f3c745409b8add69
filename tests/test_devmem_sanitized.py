"""The owners of the library's device and page-locked memory (csrc/smm_devmem.hpp) under AddressSanitizer + UBSan on
the CPU: tests/cpp/devmem_harness.cpp stands in for the seven HIP functions the header calls (malloc-backed, counting
live blocks, failing the k-th call on request) and walks alloc / upload / move / reset and the upload-then-move
sequences of smm_device.hip with every one of their HIP calls failing in turn."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_device_and_pinned_buffers_under_sanitizers(tmp_path):
    """A failed step leaves the buffer empty and the "handle" exactly as it was, no block is freed twice (the stand-in
    hipFree checks) or left behind (live-block count, LeakSanitizer), the sticky error is cleared."""
    exe = str(tmp_path / "devmem_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "devmem_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    print(out.stdout)
    assert lines[-1] == "DEVMEMBAD 0", out.stdout[-3000:]
    calls = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("SEQ")}
    # HIP calls per sequence, each failed in turn: ensure_sb = 4 x (hipMalloc + hipMemcpy) + the handle's 4 x hipFree;
    # set_epilogue = 2 uploads + the descriptor copy + 2 old vectors + the handle's 3; a pair grown = 2 x (free, alloc) + 2
    assert calls["ensure_sb"] == 12 and calls["ensure_sb_empty"] == 9
    assert calls["set_epilogue_replace"] == 10 and calls["grow_device_pair"] == 6 and calls["grow_pinned_pair"] == 6
    assert set(calls) >= {"device_basics", "pinned_basics", "set_epilogue_drop_mask", "set_epilogue_first"}
