"""CPU-only checks of PhysicalUnaryExpr (abs / sin / cos / tan over Float64, src/physical_plan/expression/unary.rs): the flat
encoding, the agreement of the four places that spell the new constants (include/nqe.h, arrow_host.py, host/naive_db.hpp,
integration/rust/gpu.rs), and the run-time generators' programs with one-operand steps compiled for gfx950 offline."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REFERENCE_ORDER = ["Abs", "Sin", "Cos", "Tan", "Trim", "LTrim", "RTrim", "CharacterLength", "Lower", "Upper", "Repeat", "Replace", "Reverse", "Substr"]


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_unary_operator_has_the_references_fourteen_names_in_order():
    from naive_query_engine_amd import UnaryOperator

    assert [m.name for m in UnaryOperator] == REFERENCE_ORDER
    assert [int(m) for m in UnaryOperator] == list(range(14))


def test_flatten_is_post_order_with_one_node_of_kind_3():
    from naive_query_engine_amd import Operator, PhysicalUnaryExpr, UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_BINARY, EXPR_COLUMN, EXPR_LITERAL, EXPR_UNARY
    from naive_query_engine_amd.expression import binop, col, lit_f64, unop
    from tests.helpers import fields

    f = fields("id", "v")
    assert EXPR_UNARY == 3
    for func in UnaryOperator:
        # name and return_type are taken and ignored, as the reference's evaluate ignores them (the planner passes "todo" / Int32)
        nodes = PhysicalUnaryExpr.create(col("v"), func, "todo", "Int32").flatten(f)
        assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_UNARY, int(func), 0)]
    # sin(v - 50.0) * 2.0 > abs(v): children first, each unary node right behind its operand's subtree
    e = binop(binop(unop(UnaryOperator.Sin, binop(col("v"), Operator.Minus, lit_f64(50.0))), Operator.Multiply, lit_f64(2.0)), Operator.Gt,
              unop(UnaryOperator.Abs, col(1)))
    got = [(n.kind, n.op) for n in e.flatten(f)]
    assert got == [(EXPR_COLUMN, 0), (EXPR_LITERAL, 0), (EXPR_BINARY, int(Operator.Minus)), (EXPR_UNARY, int(UnaryOperator.Sin)), (EXPR_LITERAL, 0),
                   (EXPR_BINARY, int(Operator.Multiply)), (EXPR_COLUMN, 0), (EXPR_UNARY, int(UnaryOperator.Abs)), (EXPR_BINARY, int(Operator.Gt))]
    assert e.referenced_columns(f) == [1, 1]


def test_header_python_cpp_and_rust_agree_on_the_new_constants():
    from naive_query_engine_amd import UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_UNARY

    header = read("include", "nqe.h")
    assert int(re.search(r"NQE_EXPR_UNARY\s*=\s*(\d+)", header).group(1)) == EXPR_UNARY == 3
    assert re.search(r"#define\s+NQE_ABI_VERSION\s+1\b", header)
    enum = re.search(r"typedef enum nqe_unary_operator \{(.*?)\} nqe_unary_operator;", header, flags=re.S).group(1)
    c_values = [(n, int(v)) for n, v in re.findall(r"NQE_UNARY_([A-Z_]+)\s*=\s*(\d+)", enum)]
    assert [n.replace("_", "") for n, _ in c_values] == [n.upper() for n in REFERENCE_ORDER]
    assert [v for _, v in c_values] == [int(m) for m in UnaryOperator]
    # the C++ mirror: an enum class in declaration order, flattened as int32_t(func) into a node of kind NQE_EXPR_UNARY
    cpp = read("naive_query_engine_amd", "host", "naive_db.hpp")
    cpp_enum = re.search(r"enum class UnaryOperator \{(.*?)\};", cpp).group(1)
    assert [n.strip() for n in cpp_enum.split(",")] == REFERENCE_ORDER
    assert "n.kind = NQE_EXPR_UNARY;" in cpp and "n.op = int32_t(func);" in cpp
    # the Rust shim: the kind constant, the operator through `as i32` of the reference's enum, whose order the comment restates
    rust = read("integration", "rust", "gpu.rs")
    assert int(re.search(r"const NQE_EXPR_UNARY: i32 = (\d+);", rust).group(1)) == 3
    assert "kind: NQE_EXPR_UNARY, op: u.func.clone() as i32" in rust
    listed = re.findall(r"\b([A-Za-z]+) = (\d+)", re.search(r"// nqe_expr_kind; nqe_unary_operator.*?\n.*?\n", rust).group(0))
    assert [(n, int(v)) for n, v in listed] == [(n, i) for i, n in enumerate(REFERENCE_ORDER)]
    assert "cast / unary" not in rust  # the cast is the only expression kind left without a device form
    assert subprocess.run(["python", os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True).returncode == 0


def test_generated_kernels_with_unary_steps_compile_offline(tmp_path, capsys):
    out = subprocess.run([os.path.join(ROOT, "tools", "jit_offline", "run.sh"), str(tmp_path), "unary"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"(\S+) (\S+)s vgprs=(\d+) vgpr_spills=(\d+) scratch=(\d+)", line)
        if m:
            rows[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)))
    with capsys.disabled():
        for name, (vgprs, spills, scratch) in rows.items():
            print(f"\n  {name}: vgprs={vgprs} vgpr_spills={spills} scratch={scratch}", end="")
    assert set(rows) == {"nqe_jit_expr_sin", "nqe_jit_expr_abs_nulls", "nqe_jit_proj_abs", "nqe_jit_selproj_abs", "nqe_jit_agg_cos", "nqe_jit_agg_abs"}, out.stdout
    for name in ("nqe_jit_agg_cos", "nqe_jit_agg_abs"):  # 1024-thread workgroups: more than 128 VGPRs cannot launch
        assert 0 < rows[name][0] <= 128, (name, rows[name])
    for name in ("nqe_jit_expr_abs_nulls", "nqe_jit_proj_abs", "nqe_jit_selproj_abs", "nqe_jit_agg_abs"):  # abs is one `and`: nothing may spill
        assert rows[name][1] == 0 and rows[name][2] == 0, (name, rows[name])
    # the sin / cos programs: registers, spills and scratch are printed above and recorded in DESIGN.md §3.6 (the math library's
    # code under the aggregate kernel's 128-register cap spills; that is reported, not asserted away)
    src = (tmp_path / "nqe_jit_expr_sin.hip").read_text()
    assert "d2u(sin(u2d(a)))" in src and "#pragma clang fp contract(off)" in src and "__sinf" not in src and "native_" not in src
    assert "d2u(cos(u2d(a)))" in (tmp_path / "nqe_jit_agg_cos.hip").read_text()
    assert "a & 0x7fffffffffffffffull" in (tmp_path / "nqe_jit_selproj_abs.hip").read_text()
