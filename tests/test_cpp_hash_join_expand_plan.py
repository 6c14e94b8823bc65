"""The column list of the join's count -> scan -> expand-and-write path (naive_query_engine_amd/csrc/hash_join_expand_plan.hpp: which
kernel column reads what and lands where, for the inner probe of a duplicate-key table and for the outer probe, and the PLAIN verdict)
on the CPU: tests/cpp/test_hash_join_expand_plan.cpp includes that header alone, is compiled with g++ and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_join_expand_plan(tmp_path):
    exe = str(tmp_path / "test_hash_join_expand_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_hash_join_expand_plan.cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "naive_query_engine_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "hash join expand plan ok" in out.stdout, out.stdout + out.stderr
