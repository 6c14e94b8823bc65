"""The rules of the string functions with arguments (naive_query_engine_amd/csrc/string_args_parts.hpp, quirk Q26: SUBSTR's window and
character positions, REPEAT's and REPLACE's saturating lengths, the border test, the greedy resolution of a chunk's candidates and the
placement of every byte) on the CPU: tests/cpp/test_string_args.cpp includes that header alone, is compiled with g++ and runs every byte
string of up to 7 bytes over a six-byte alphabet against a sequential reference — once plain, once as a stand-alone executable built with
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_string_args.cpp")
FLAGS = ["-O2", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc")]
OK = "string args ok: 335993 strings"  # 335923 of up to 7 bytes, 60 random longer ones, 10 runs for the bordered patterns


def test_string_args_rules(tmp_path):
    exe = str(tmp_path / "test_string_args")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and OK in out.stdout, out.stdout + out.stderr


def test_string_args_rules_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_string_args_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and OK in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr
