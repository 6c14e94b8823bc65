"""CPU-only checks of PhysicalStringArgsExpr (quirk Q26: NQE_EXPR_STRING_ARGS): the flat encoding, the agreement of the four places that
spell the new constant (include/nqe.h, arrow_host.py, host/naive_db.hpp, integration/rust/gpu.rs), the static dtype of the Python
mirror, the exports, and that PhysicalStringExpr and PhysicalUnaryExpr encode what they always did."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_flatten_is_post_order_with_the_children_left_to_right():
    from naive_query_engine_amd import DType, Operator, PhysicalStringArgsExpr, UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_BINARY, EXPR_COLUMN, EXPR_LITERAL, EXPR_STRING, EXPR_STRING_ARGS
    from naive_query_engine_amd.expression import INT64_MAX, binop, col, lit_i64, lit_utf8, repeat, replace, strop, substr
    from tests.helpers import fields

    f = fields("id", "s")
    assert EXPR_STRING_ARGS == 5 and INT64_MAX == 2 ** 63 - 1
    nodes = substr(col("s"), 1, 2).flatten(f)
    assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_LITERAL, 0, 0), (EXPR_LITERAL, 0, 0), (EXPR_STRING_ARGS, int(UnaryOperator.Substr), 0)]
    assert [nodes[1].value.i64, nodes[2].value.i64] == [1, 2] and nodes[1].dtype == int(DType.INT64)     # the string deepest, the last argument on top
    nodes = substr(col("s"), 3).flatten(f)                                                                 # to the end: Int64 max, no two-operand form
    assert len(nodes) == 4 and nodes[2].value.i64 == INT64_MAX and nodes[1].value.i64 == 3
    nodes = repeat(col("s"), col("id")).flatten(f)
    assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_COLUMN, 0, 0), (EXPR_STRING_ARGS, int(UnaryOperator.Repeat), 0)]
    nodes = replace(col("s"), "-", " ").flatten(f)
    assert [(n.kind, n.op) for n in nodes] == [(EXPR_COLUMN, 0), (EXPR_LITERAL, 0), (EXPR_LITERAL, 0), (EXPR_STRING_ARGS, int(UnaryOperator.Replace))]
    assert [n.dtype for n in nodes[1:3]] == [int(DType.UTF8)] * 2 and [n.utf8_length for n in nodes[1:3]] == [1, 1]
    # any operator and any number of arguments are encoded as they are: the library decides
    for func in UnaryOperator:
        nodes = PhysicalStringArgsExpr.create(func, col("s"), [lit_i64(1)] * 3).flatten(f)
        assert len(nodes) == 5 and (nodes[-1].kind, nodes[-1].op) == (EXPR_STRING_ARGS, int(func))
    # character_length(replace(s, ' ', '')) and substr(s, character_length(s) - 1, 2) = 'ab': each node right behind its last child's subtree
    e = strop(UnaryOperator.CharacterLength, replace(col("s"), " ", ""))
    assert [(n.kind, n.op) for n in e.flatten(f)] == [(EXPR_COLUMN, 0), (EXPR_LITERAL, 0), (EXPR_LITERAL, 0), (EXPR_STRING_ARGS, int(UnaryOperator.Replace)),
                                                     (EXPR_STRING, int(UnaryOperator.CharacterLength))]
    e = binop(substr(col("s"), binop(strop(UnaryOperator.CharacterLength, col("s")), Operator.Minus, lit_i64(1)), 2), Operator.Eq, lit_utf8("ab"))
    assert [(n.kind, n.op) for n in e.flatten(f)] == [(EXPR_COLUMN, 0), (EXPR_COLUMN, 0), (EXPR_STRING, int(UnaryOperator.CharacterLength)), (EXPR_LITERAL, 0),
                                                     (EXPR_BINARY, int(Operator.Minus)), (EXPR_LITERAL, 0), (EXPR_STRING_ARGS, int(UnaryOperator.Substr)), (EXPR_LITERAL, 0),
                                                     (EXPR_BINARY, int(Operator.Eq))]
    assert repeat(substr(col("s"), col("id"), 2), col("id")).referenced_columns(f) == [1, 0, 0]            # over all children
    assert repr(substr(col("s"), 1, 2)).startswith("Substr(ColumnExpr(") and repr(replace(col(1), "a", "b")).startswith("Replace(")


def test_string_and_unary_exprs_flatten_as_before():
    from naive_query_engine_amd import PhysicalStringExpr, PhysicalUnaryExpr, UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_COLUMN, EXPR_STRING, EXPR_UNARY
    from naive_query_engine_amd.expression import col
    from tests.helpers import fields

    for func in UnaryOperator:
        nodes = PhysicalUnaryExpr.create(col("v"), func, "todo", "Int32").flatten(fields("id", "v"))
        assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_UNARY, int(func), 0)]
        nodes = PhysicalStringExpr.create(col("v"), func).flatten(fields("id", "v"))
        assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_STRING, int(func), 0)]


def test_header_python_cpp_and_rust_agree_on_the_new_constant():
    from naive_query_engine_amd.arrow_host import EXPR_STRING_ARGS

    header = read("include", "nqe.h")
    assert int(re.search(r"NQE_EXPR_STRING_ARGS\s*=\s*(\d+)", header).group(1)) == EXPR_STRING_ARGS == 5
    assert re.search(r"#define\s+NQE_ABI_VERSION\s+1\b", header)
    kinds = re.search(r"typedef enum nqe_expr_kind \{(.*?)\} nqe_expr_kind;", header, flags=re.S).group(1)
    assert [(n, int(v)) for n, v in re.findall(r"NQE_EXPR_([A-Z_]+)\s*=\s*(\d+)", kinds)] == [("COLUMN", 0), ("LITERAL", 1), ("BINARY", 2), ("UNARY", 3), ("STRING", 4),
                                                                                            ("STRING_ARGS", 5)]
    assert "nqe_string_operator" not in header and len(re.findall(r"typedef enum nqe_unary_operator", header)) == 1
    cpp = read("naive_query_engine_amd", "host", "naive_db.hpp")
    assert "struct PhysicalStringArgsExpr : PhysicalExpr" in cpp and "n.kind = NQE_EXPR_STRING_ARGS;" in cpp
    body = cpp[cpp.index("struct PhysicalStringArgsExpr"):]
    body = body[:body.index("\n};")]
    assert "n.op = int32_t(func);" in body and "UnaryOperator func;" in body and "std::vector<PhysicalExprRef> args;" in body
    assert "n.kind == NQE_EXPR_STRING_ARGS" in cpp  # the static-type stack walk pops the node's arity
    rust = read("integration", "rust", "gpu.rs")
    assert int(re.search(r"const NQE_EXPR_STRING_ARGS: i32 = (\d+);", rust).group(1)) == 5
    assert "pub struct PhysicalStringArgsExpr" in rust and "impl PhysicalExpr for PhysicalStringArgsExpr" in rust
    assert "kind: NQE_EXPR_STRING_ARGS, op: s.func.clone() as i32" in rust
    assert subprocess.run(["python", os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True).returncode == 0


def test_static_dtype_of_the_python_mirror():
    from naive_query_engine_amd import DType, Field, Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_utf8, repeat, replace, strop, substr
    from naive_query_engine_amd.physical_plan import _static_dtype

    schema = [Field("id", DType.INT64, False), Field("s", DType.UTF8, True), Field("v", DType.FLOAT64, False)]
    for e in (substr(col("s"), 1, 2), substr(col("s"), col("id")), repeat(col("s"), col("id")), replace(col("s"), "a", "b"), repeat(lit_utf8("x"), 3),
              substr(strop(UnaryOperator.Trim, col("s")), 2, 2), replace(substr(col("s"), 1, 2), "a", "")):
        assert _static_dtype(e, schema) == DType.UTF8
    assert _static_dtype(strop(UnaryOperator.CharacterLength, replace(col("s"), " ", "")), schema) == DType.INT64
    assert _static_dtype(binop(substr(col("s"), 1, 2), Operator.Eq, lit_utf8("DE")), schema) == DType.BOOLEAN
    assert _static_dtype(strop(UnaryOperator.Lower, col("s")), schema) == DType.UTF8 and _static_dtype(col("v"), schema) == DType.FLOAT64  # what was there


def test_the_package_exports_the_node():
    import naive_query_engine_amd as pkg

    assert "PhysicalStringArgsExpr" in pkg.__all__ and pkg.PhysicalStringArgsExpr.create is not None
    assert "PhysicalStringExpr" in pkg.__all__ and "PhysicalUnaryExpr" in pkg.__all__
    assert pkg.expression.STRING_ARGS_FUNCTIONS == tuple(pkg.UnaryOperator[n] for n in ("Repeat", "Replace", "Substr"))
    assert len(pkg.expression.STRING_FUNCTIONS) == 7 and not set(pkg.expression.STRING_FUNCTIONS) & set(pkg.expression.STRING_ARGS_FUNCTIONS)
