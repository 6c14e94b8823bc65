"""CPU-only checks of PhysicalConditionalExpr (quirk Q28: NQE_EXPR_CONDITIONAL): the flat encoding (kind 7, the operator, `column` equal to
the number of operands, the operands in order), the nesting of the helpers, the static dtype of the Python mirror, the exports, the
agreement of the five places that spell the new constant (include/nqe.h, arrow_host.py, host/naive_db.hpp, integration/rust/gpu.rs,
INTEGRATION.md), and the Rust shim check."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_flatten_carries_the_arity_and_the_operands_in_order():
    from naive_query_engine_amd import CondOperator, DType, Operator, PhysicalConditionalExpr
    from naive_query_engine_amd import expression as e
    from naive_query_engine_amd.arrow_host import EXPR_BINARY, EXPR_COLUMN, EXPR_CONDITIONAL, EXPR_LITERAL, node_conditional
    from tests.helpers import fields

    f = fields("id", "v", "b", "s")
    col = e.col
    assert EXPR_CONDITIONAL == 7
    assert [(m.name, int(m)) for m in CondOperator] == [("Not", 0), ("IsNull", 1), ("IsNotNull", 2), ("Coalesce", 3), ("NullIf", 4), ("If", 5)]
    assert e.COND_ARITY == {CondOperator.Not: 1, CondOperator.IsNull: 1, CondOperator.IsNotNull: 1, CondOperator.Coalesce: 2, CondOperator.NullIf: 2, CondOperator.If: 3}
    n = node_conditional(CondOperator.If, 3)
    assert (n.kind, n.op, n.column) == (7, 5, 3)
    for helper, op, name in [(e.not_, CondOperator.Not, "b"), (e.is_null, CondOperator.IsNull, "s"), (e.is_not_null, CondOperator.IsNotNull, "v")]:
        nodes = helper(col(name)).flatten(f)
        assert [(x.kind, x.op, x.column) for x in nodes] == [(EXPR_COLUMN, 0, [y.name for y in f].index(name)), (EXPR_CONDITIONAL, int(op), 1)]
    for helper, op in [(e.coalesce, CondOperator.Coalesce), (e.nullif, CondOperator.NullIf)]:
        nodes = helper(col("id"), e.lit_i64(-1)).flatten(f)
        assert [(x.kind, x.op, x.column) for x in nodes] == [(EXPR_COLUMN, 0, 0), (EXPR_LITERAL, 0, 0), (EXPR_CONDITIONAL, int(op), 2)]
        assert nodes[1].value.i64 == -1
    # if_else: the condition deepest, the else value on top
    nodes = e.if_else(e.binop(col("v"), Operator.Gt, e.lit_f64(50.0)), e.lit_i64(1), e.lit_i64(0)).flatten(f)
    assert [(x.kind, x.op, x.column) for x in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_LITERAL, 0, 0), (EXPR_BINARY, int(Operator.Gt), 0), (EXPR_LITERAL, 0, 0), (EXPR_LITERAL, 0, 0),
                                                         (EXPR_CONDITIONAL, int(CondOperator.If), 3)]
    assert nodes[3].value.i64 == 1 and nodes[4].value.i64 == 0
    # any number of operands is encoded as it is: the library refuses it
    nodes = PhysicalConditionalExpr.create(CondOperator.Not, [col("b"), col("b")]).flatten(f)
    assert (nodes[-1].kind, nodes[-1].op, nodes[-1].column) == (7, 0, 2)
    assert PhysicalConditionalExpr.create(CondOperator.If, []).flatten(f)[-1].column == 0
    # lit_null: ScalarValue::X(None) of the type
    for dt in (DType.INT64, DType.UINT64, DType.FLOAT64, DType.BOOLEAN, DType.UTF8):
        (n,) = e.lit_null(dt).flatten(f)
        assert (n.kind, n.dtype, n.is_null) == (EXPR_LITERAL, int(dt), 1)
    assert e.coalesce(col("s"), e.lit_utf8("x")).referenced_columns(f) == [3]
    assert repr(e.coalesce(col("id"), e.lit_i64(0))).startswith("Coalesce(ColumnExpr(") and repr(e.not_(col("b"))).startswith("Not(")


def test_the_helpers_nest():
    from naive_query_engine_amd import CondOperator
    from naive_query_engine_amd import expression as e
    from naive_query_engine_amd.arrow_host import EXPR_COLUMN, EXPR_CONDITIONAL, EXPR_LITERAL
    from tests.helpers import fields

    f = fields("a", "b", "c", "c1", "c2")
    col = e.col
    C, IF = int(CondOperator.Coalesce), int(CondOperator.If)
    # coalesce(a, b, c) = a b c COALESCE COALESCE
    nodes = e.coalesce(col("a"), col("b"), col("c")).flatten(f)
    assert [(x.kind, x.op, x.column) for x in nodes] == [(EXPR_COLUMN, 0, 0), (EXPR_COLUMN, 0, 1), (EXPR_COLUMN, 0, 2), (EXPR_CONDITIONAL, C, 2), (EXPR_CONDITIONAL, C, 2)]
    nodes = e.coalesce(col("a"), col("b"), col("c"), e.lit_i64(0)).flatten(f)
    assert [(x.kind, x.op) for x in nodes][-3:] == [(EXPR_CONDITIONAL, C)] * 3 and len(nodes) == 7
    # CASE WHEN c1 THEN a WHEN c2 THEN b ELSE c END = c1 a c2 b c IF IF
    nodes = e.case_when([(col("c1"), col("a")), (col("c2"), col("b"))], col("c")).flatten(f)
    assert [(x.kind, x.op, x.column) for x in nodes] == [(EXPR_COLUMN, 0, 3), (EXPR_COLUMN, 0, 0), (EXPR_COLUMN, 0, 4), (EXPR_COLUMN, 0, 1), (EXPR_COLUMN, 0, 2),
                                                         (EXPR_CONDITIONAL, IF, 3), (EXPR_CONDITIONAL, IF, 3)]
    # without ELSE: the NULL literal of the value type
    from naive_query_engine_amd import DType

    nodes = e.case_when([(col("c1"), col("a"))], e.lit_null(DType.INT64)).flatten(f)
    assert [(x.kind, x.is_null) for x in nodes] == [(EXPR_COLUMN, 0), (EXPR_COLUMN, 0), (EXPR_LITERAL, 1), (EXPR_CONDITIONAL, 0)]
    assert e.case_when([], col("c")).flatten(f)[0].column == 2  # no WHEN: the ELSE value itself
    # a reader walks the stack by `column` alone
    depth = 0
    for x in e.case_when([(e.is_null(col("a")), e.coalesce(col("b"), col("c")))], e.nullif(col("a"), col("b"))).flatten(f):
        depth += 1 - (x.column if x.kind == EXPR_CONDITIONAL else 0)
    assert depth == 1


def test_static_dtype_and_exports():
    import naive_query_engine_amd as pkg
    from naive_query_engine_amd import DType, Field, Operator
    from naive_query_engine_amd import expression as e

    for name in ("PhysicalConditionalExpr", "CondOperator"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("not_", "is_null", "is_not_null", "coalesce", "nullif", "if_else", "case_when", "lit_null"):
        assert callable(getattr(e, name))
    src = read("naive_query_engine_amd", "physical_plan.py")
    assert "PhysicalConditionalExpr" in src and "CondOperator" in src
    # (_static_dtype lives in physical_plan.py, which loads the library: exercised where the library is built)
    lib = os.path.join(ROOT, "naive_query_engine_amd", "libnqe_hip.so")
    if os.path.exists(lib):
        from naive_query_engine_amd.physical_plan import _static_dtype

        schema = [Field("id", DType.INT64, True), Field("v", DType.FLOAT64, True), Field("b", DType.BOOLEAN, True), Field("s", DType.UTF8, True)]
        col = e.col
        assert _static_dtype(e.not_(col("b")), schema) == DType.BOOLEAN
        assert _static_dtype(e.is_null(col("s")), schema) == DType.BOOLEAN and _static_dtype(e.is_not_null(col("v")), schema) == DType.BOOLEAN
        assert _static_dtype(e.coalesce(col("s"), e.lit_utf8("unknown")), schema) == DType.UTF8
        assert _static_dtype(e.nullif(col("id"), e.lit_i64(0)), schema) == DType.INT64
        assert _static_dtype(e.if_else(e.binop(col("v"), Operator.Gt, e.lit_f64(0.0)), e.lit_i64(1), e.lit_i64(0)), schema) == DType.INT64
        assert _static_dtype(e.case_when([(col("b"), col("v"))], e.lit_null(DType.FLOAT64)), schema) == DType.FLOAT64
        assert _static_dtype(e.coalesce(col("v"), col("v"), e.lit_f64(0.0)), schema) == DType.FLOAT64


def test_the_five_places_agree_on_the_new_constant_and_the_enum():
    from naive_query_engine_amd import CondOperator
    from naive_query_engine_amd.arrow_host import EXPR_CONDITIONAL

    header = read("include", "nqe.h")
    assert re.search(r"#define\s+NQE_ABI_VERSION\s+1\b", header)
    assert int(re.search(r"#define\s+NQE_EXPR_CONDITIONAL\s+(\d+)\b", header).group(1)) == EXPR_CONDITIONAL == 7
    kinds = re.search(r"typedef enum nqe_expr_kind \{(.*?)\} nqe_expr_kind;", header, flags=re.S).group(1)
    assert "CONDITIONAL" not in kinds  # the enum's list is frozen: the kind is a #define beside it, held by a compile-time check
    assert re.search(r"typedef char \w+\[\(NQE_EXPR_CONDITIONAL == NQE_EXPR_STRING_MATCH \+ 1\) \? 1 : -1\];", header)
    ops = re.search(r"typedef enum nqe_cond_operator \{(.*?)\} nqe_cond_operator;", header, flags=re.S).group(1)
    pairs = [(n, int(v)) for n, v in re.findall(r"NQE_COND_([A-Z_]+)\s*=\s*(\d+)", ops)]
    assert pairs == [("NOT", 0), ("IS_NULL", 1), ("IS_NOT_NULL", 2), ("COALESCE", 3), ("NULLIF", 4), ("IF", 5)]
    assert [(m.name.upper(), int(m)) for m in CondOperator] == [(n.replace("_", ""), v) for n, v in pairs]
    cpp = read("naive_query_engine_amd", "host", "naive_db.hpp")
    assert "struct PhysicalConditionalExpr : PhysicalExpr" in cpp and "n.kind = NQE_EXPR_CONDITIONAL;" in cpp and "n.column = int32_t(operands.size());" in cpp
    assert "constexpr int32_t EXPR_CONDITIONAL = NQE_EXPR_CONDITIONAL;" in cpp and "static_assert(EXPR_CONDITIONAL == 7" in cpp
    assert "enum class CondOperator : int32_t { Not = 0, IsNull = 1, IsNotNull = 2, Coalesce = 3, NullIf = 4, If = 5 }" in cpp
    assert "n.kind == NQE_EXPR_CONDITIONAL" in cpp  # the static-type stack walk pops the node's `column` values
    rust = read("integration", "rust", "gpu.rs")
    assert int(re.search(r"const NQE_EXPR_CONDITIONAL: i32 = (\d+);", rust).group(1)) == 7
    assert "pub struct PhysicalConditionalExpr" in rust and "impl PhysicalExpr for PhysicalConditionalExpr" in rust
    assert "pub enum CondOperator { Not = 0, IsNull = 1, IsNotNull = 2, Coalesce = 3, NullIf = 4, If = 5 }" in rust
    assert "kind: NQE_EXPR_CONDITIONAL, op: c.op as i32, column: c.operands.len() as i32" in rust
    doc = read("INTEGRATION.md")
    assert "NQE_EXPR_CONDITIONAL" in doc and re.search(r"NQE_EXPR_CONDITIONAL\W+=?\W*7\b", doc) and "PhysicalConditionalExpr" in doc
    for name in ("DESIGN.md", "SURVEY.md", "README.md"):
        assert "Q28" in read(name), name
    assert "§3.22" in read("DESIGN.md") or "3.22" in read("DESIGN.md")
    # the kernels' unit is built and checked for spills
    assert "conditional.hip" in read("naive_query_engine_amd", "csrc", "Makefile") and "conditional.hip" in read("tools", "check_spills.sh")


def test_the_rust_shim_check_passes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
