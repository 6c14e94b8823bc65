"""The rules of the string functions (naive_query_engine_amd/csrc/string_fn_parts.hpp, quirk Q25: trim ranges, the byte and word case
maps, unit starts and destinations of REVERSE, the non-continuation count) on the CPU: tests/cpp/test_string_fn.cpp includes that
header alone, is compiled with g++ and runs every byte string of up to 7 bytes over a six-byte alphabet against a sequential reference."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_string_fn_rules(tmp_path):
    exe = str(tmp_path / "test_string_fn")
    src = os.path.join(ROOT, "tests", "cpp", "test_string_fn.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "string fn ok: 335923 strings" in out.stdout, out.stdout + out.stderr
