"""The per-row rules of the conditional and NULL-handling functions (naive_query_engine_amd/csrc/conditional_parts.hpp, quirk Q28: what
NOT, IS_NULL, IS_NOT_NULL, COALESCE, NULLIF and IF make of one row's words and of 64 rows' bits, the tail mask, the source of a Utf8
row) on the CPU: tests/cpp/test_conditional.cpp includes that header alone, is compiled with g++ and decides every combination against a
restatement of its own — once plain, once as a stand-alone executable built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_conditional.cpp")
FLAGS = ["-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc")]
OK = "conditional ok: "


def test_conditional_rules(tmp_path):
    exe = str(tmp_path / "test_conditional")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and OK in out.stdout, out.stdout + out.stderr


def test_conditional_rules_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_conditional_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and OK in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
