"""Who owns the library's device and pinned memory (gorder_amd/csrc/device_mem.h), without a GPU: the owning buffer and the
replica rule driven by a stand-alone program with a counting allocator, under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owning_buffer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "device_mem")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'gorder_amd', 'csrc')}",
                           os.path.join(ROOT, "tests", "cabi", "device_mem.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "device_mem ok" in res.stdout and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
