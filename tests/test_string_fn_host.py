"""CPU-only checks of PhysicalStringExpr (quirk Q25: NQE_EXPR_STRING): the flat encoding, the agreement of the four places that spell
the new constant (include/nqe.h, arrow_host.py, host/naive_db.hpp, integration/rust/gpu.rs), the static dtype of the Python mirror,
the Rust shim's drift check, and that PhysicalUnaryExpr encodes what it always did."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_flatten_is_post_order_with_one_node_of_kind_4():
    from naive_query_engine_amd import Operator, PhysicalStringExpr, UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_BINARY, EXPR_COLUMN, EXPR_LITERAL, EXPR_STRING, EXPR_UNARY
    from naive_query_engine_amd.expression import binop, col, lit_i64, lit_utf8, strop
    from tests.helpers import fields

    f = fields("id", "s")
    assert EXPR_STRING == 4 and EXPR_UNARY == 3
    for func in UnaryOperator:  # any operator is encoded as it is: the library decides
        nodes = PhysicalStringExpr.create(col("s"), func).flatten(f)
        assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_STRING, int(func), 0)]
    # lower(trim(s)) = 'bob' and character_length(s) * 2 > id: children first, each string node right behind its operand's subtree
    e = binop(strop(UnaryOperator.Lower, strop(UnaryOperator.Trim, col("s"))), Operator.Eq, lit_utf8("bob"))
    assert [(n.kind, n.op) for n in e.flatten(f)] == [(EXPR_COLUMN, 0), (EXPR_STRING, int(UnaryOperator.Trim)), (EXPR_STRING, int(UnaryOperator.Lower)), (EXPR_LITERAL, 0),
                                                     (EXPR_BINARY, int(Operator.Eq))]
    e = binop(binop(strop(UnaryOperator.CharacterLength, col(1)), Operator.Multiply, lit_i64(2)), Operator.Gt, col(0))
    assert [(n.kind, n.op) for n in e.flatten(f)] == [(EXPR_COLUMN, 0), (EXPR_STRING, int(UnaryOperator.CharacterLength)), (EXPR_LITERAL, 0), (EXPR_BINARY, int(Operator.Multiply)),
                                                     (EXPR_COLUMN, 0), (EXPR_BINARY, int(Operator.Gt))]
    assert e.referenced_columns(f) == [1, 0]
    assert repr(strop(UnaryOperator.Reverse, col("s"))).startswith("Reverse(")


def test_unary_expr_flattens_as_before():
    from naive_query_engine_amd import PhysicalUnaryExpr, UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_COLUMN, EXPR_UNARY
    from naive_query_engine_amd.expression import col
    from tests.helpers import fields

    for func in UnaryOperator:
        nodes = PhysicalUnaryExpr.create(col("v"), func, "todo", "Int32").flatten(fields("id", "v"))
        assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_UNARY, int(func), 0)]


def test_header_python_cpp_and_rust_agree_on_the_new_constant():
    from naive_query_engine_amd.arrow_host import EXPR_STRING

    header = read("include", "nqe.h")
    assert int(re.search(r"NQE_EXPR_STRING\s*=\s*(\d+)", header).group(1)) == EXPR_STRING == 4
    assert re.search(r"#define\s+NQE_ABI_VERSION\s+1\b", header)
    kinds = re.search(r"typedef enum nqe_expr_kind \{(.*?)\} nqe_expr_kind;", header, flags=re.S).group(1)
    assert [(n, int(v)) for n, v in re.findall(r"NQE_EXPR_([A-Z]+)\s*=\s*(\d+)", kinds)] == [("COLUMN", 0), ("LITERAL", 1), ("BINARY", 2), ("UNARY", 3), ("STRING", 4)]
    # no second enum: the node's op is a nqe_unary_operator
    assert "nqe_string_operator" not in header and len(re.findall(r"typedef enum nqe_unary_operator", header)) == 1
    cpp = read("naive_query_engine_amd", "host", "naive_db.hpp")
    assert "struct PhysicalStringExpr : PhysicalExpr" in cpp and "n.kind = NQE_EXPR_STRING;" in cpp
    body = cpp[cpp.index("struct PhysicalStringExpr"):]
    body = body[:body.index("\n};")]
    assert "n.op = int32_t(func);" in body and "UnaryOperator func;" in body
    assert "struct PhysicalUnaryExpr : PhysicalExpr { // unary.rs:46-109" in cpp and "n.kind = NQE_EXPR_UNARY;" in cpp
    rust = read("integration", "rust", "gpu.rs")
    assert int(re.search(r"const NQE_EXPR_STRING: i32 = (\d+);", rust).group(1)) == 4
    assert "pub struct PhysicalStringExpr" in rust and "impl PhysicalExpr for PhysicalStringExpr" in rust
    assert "kind: NQE_EXPR_STRING, op: s.func.clone() as i32" in rust
    assert "kind: NQE_EXPR_UNARY, op: u.func.clone() as i32" in rust  # PhysicalUnaryExpr untouched
    assert subprocess.run(["python", os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True).returncode == 0


def test_static_dtype_of_the_python_mirror():
    from naive_query_engine_amd import DType, Field, Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_i64, lit_utf8, strop, unop
    from naive_query_engine_amd.physical_plan import _static_dtype

    schema = [Field("id", DType.INT64, False), Field("s", DType.UTF8, True), Field("v", DType.FLOAT64, False)]
    for func in (UnaryOperator.Trim, UnaryOperator.LTrim, UnaryOperator.RTrim, UnaryOperator.Lower, UnaryOperator.Upper, UnaryOperator.Reverse):
        assert _static_dtype(strop(func, col("s")), schema) == DType.UTF8
    assert _static_dtype(strop(UnaryOperator.CharacterLength, col("s")), schema) == DType.INT64
    assert _static_dtype(strop(UnaryOperator.Lower, strop(UnaryOperator.Trim, lit_utf8("x"))), schema) == DType.UTF8
    assert _static_dtype(binop(strop(UnaryOperator.CharacterLength, col("s")), Operator.Multiply, lit_i64(2)), schema) == DType.INT64
    assert _static_dtype(binop(strop(UnaryOperator.Lower, col("s")), Operator.Eq, lit_utf8("bob")), schema) == DType.BOOLEAN
    # what was there: a column, a literal, a unary function
    assert _static_dtype(col("s"), schema) == DType.UTF8 and _static_dtype(lit_i64(1), schema) == DType.INT64
    assert _static_dtype(unop(UnaryOperator.Abs, col("v")), schema) == DType.FLOAT64


def test_the_package_exports_the_node():
    import naive_query_engine_amd as pkg

    assert "PhysicalStringExpr" in pkg.__all__ and pkg.PhysicalStringExpr.create is not None
    assert pkg.expression.STRING_FUNCTIONS == tuple(pkg.UnaryOperator[n] for n in ("Trim", "LTrim", "RTrim", "CharacterLength", "Lower", "Upper", "Reverse"))
