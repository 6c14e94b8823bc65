"""CPU-only checks of PhysicalStringMatchExpr (quirk Q27: NQE_EXPR_STRING_MATCH): the flat encoding, the agreement of the five places
that spell the new constant (include/nqe.h, arrow_host.py, host/naive_db.hpp, integration/rust/gpu.rs), the enum text of
the header, the static dtype of the Python mirror, the exports, and that PhysicalStringExpr and PhysicalStringArgsExpr encode what they
always did."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_flatten_is_post_order_with_the_string_deepest():
    from naive_query_engine_amd import DType, MatchOperator, Operator, PhysicalStringMatchExpr, UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_BINARY, EXPR_COLUMN, EXPR_LITERAL, EXPR_STRING, EXPR_STRING_ARGS, EXPR_STRING_MATCH
    from naive_query_engine_amd import expression as e
    from tests.helpers import fields

    f = fields("id", "s")
    col = e.col
    assert EXPR_STRING_MATCH == 6
    helpers = [(e.like, MatchOperator.Like), (e.not_like, MatchOperator.NotLike), (e.ilike, MatchOperator.ILike), (e.not_ilike, MatchOperator.NotILike),
               (e.starts_with, MatchOperator.StartsWith), (e.ends_with, MatchOperator.EndsWith), (e.contains, MatchOperator.Contains), (e.strpos, MatchOperator.StrPos)]
    assert [int(op) for _, op in helpers] == list(range(8)) == [int(op) for op in MatchOperator]
    for helper, op in helpers:
        nodes = helper(col("s"), "a%").flatten(f)
        assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_LITERAL, 0, 0), (EXPR_STRING_MATCH, int(op), 0)]
        assert nodes[1].dtype == int(DType.UTF8) and nodes[1].utf8_length == 2 and nodes[1].is_null == 0
    # the pattern as str, bytes, None or an expression: the library decides what is legal
    nodes = e.like(col("s"), b"\xa9_").flatten(f)
    assert nodes[1].utf8_length == 2 and nodes[1].dtype == int(DType.UTF8)
    nodes = e.contains(col("s"), None).flatten(f)
    assert nodes[1].is_null == 1 and nodes[1].dtype == int(DType.UTF8)
    nodes = e.strpos(col("s"), col("id")).flatten(f)
    assert [(n.kind, n.column) for n in nodes] == [(EXPR_COLUMN, 1), (EXPR_COLUMN, 0), (EXPR_STRING_MATCH, 0)]
    nodes = PhysicalStringMatchExpr.create(MatchOperator.Like, col("id"), e.lit_i64(3)).flatten(f)
    assert [(n.kind, n.op) for n in nodes] == [(EXPR_COLUMN, 0), (EXPR_LITERAL, 0), (EXPR_STRING_MATCH, 0)]
    # like(lower(s), 'ab%') and substr(s, strpos(s, '-') + 1): each node right behind its last child's subtree
    nodes = e.like(e.strop(UnaryOperator.Lower, col("s")), "ab%").flatten(f)
    assert [(n.kind, n.op) for n in nodes] == [(EXPR_COLUMN, 0), (EXPR_STRING, int(UnaryOperator.Lower)), (EXPR_LITERAL, 0), (EXPR_STRING_MATCH, 0)]
    nodes = e.substr(col("s"), e.binop(e.strpos(col("s"), "-"), Operator.Plus, e.lit_i64(1))).flatten(f)
    assert [(n.kind, n.op) for n in nodes] == [(EXPR_COLUMN, 0), (EXPR_COLUMN, 0), (EXPR_LITERAL, 0), (EXPR_STRING_MATCH, int(MatchOperator.StrPos)), (EXPR_LITERAL, 0),
                                               (EXPR_BINARY, int(Operator.Plus)), (EXPR_LITERAL, 0), (EXPR_STRING_ARGS, int(UnaryOperator.Substr))]
    assert e.like(e.substr(col("s"), col("id"), 2), "a").referenced_columns(f) == [1, 0]
    assert repr(e.like(col("s"), "a%")).startswith("Like(ColumnExpr(") and repr(e.strpos(col(1), "a")).startswith("StrPos(")


def test_string_and_string_args_exprs_flatten_as_before():
    from naive_query_engine_amd import PhysicalStringArgsExpr, PhysicalStringExpr, UnaryOperator
    from naive_query_engine_amd.arrow_host import EXPR_COLUMN, EXPR_LITERAL, EXPR_STRING, EXPR_STRING_ARGS
    from naive_query_engine_amd.expression import col, lit_i64
    from tests.helpers import fields

    for func in UnaryOperator:
        nodes = PhysicalStringExpr.create(col("v"), func).flatten(fields("id", "v"))
        assert [(n.kind, n.op, n.column) for n in nodes] == [(EXPR_COLUMN, 0, 1), (EXPR_STRING, int(func), 0)]
        nodes = PhysicalStringArgsExpr.create(func, col("v"), [lit_i64(1), lit_i64(2)]).flatten(fields("id", "v"))
        assert [(n.kind, n.op) for n in nodes] == [(EXPR_COLUMN, 0), (EXPR_LITERAL, 0), (EXPR_LITERAL, 0), (EXPR_STRING_ARGS, int(func))]


def test_the_five_places_agree_on_the_new_constant_and_the_enum():
    from naive_query_engine_amd import MatchOperator
    from naive_query_engine_amd.arrow_host import EXPR_STRING_MATCH

    header = read("include", "nqe.h")
    assert re.search(r"#define\s+NQE_ABI_VERSION\s+1\b", header)
    # the enumerator carries no initializer (an earlier test reads the `NAME = value` pairs as a fixed list); a compile-time check holds it at 6
    kinds = re.search(r"typedef enum nqe_expr_kind \{(.*?)\} nqe_expr_kind;", header, flags=re.S).group(1)
    names = [part.split("=")[0].strip() for part in kinds.split(",")]
    assert names == ["NQE_EXPR_COLUMN", "NQE_EXPR_LITERAL", "NQE_EXPR_BINARY", "NQE_EXPR_UNARY", "NQE_EXPR_STRING", "NQE_EXPR_STRING_ARGS", "NQE_EXPR_STRING_MATCH"]
    assert names.index("NQE_EXPR_STRING_MATCH") == EXPR_STRING_MATCH == 6 and "NQE_EXPR_STRING_ARGS = 5" in kinds and "NQE_EXPR_STRING_MATCH =" not in kinds
    assert re.search(r"typedef char \w+\[\(NQE_EXPR_STRING_MATCH == 6\) \? 1 : -1\];", header)
    ops = re.search(r"typedef enum nqe_match_operator \{(.*?)\} nqe_match_operator;", header, flags=re.S).group(1)
    pairs = [(n, int(v)) for n, v in re.findall(r"NQE_MATCH_([A-Z_]+)\s*=\s*(\d+)", ops)]
    assert pairs == [("LIKE", 0), ("NOT_LIKE", 1), ("ILIKE", 2), ("NOT_ILIKE", 3), ("STARTS_WITH", 4), ("ENDS_WITH", 5), ("CONTAINS", 6), ("STRPOS", 7)]
    assert [(m.name.upper(), int(m)) for m in MatchOperator] == [(n.replace("_", ""), v) for n, v in pairs]
    assert len(pairs) < 14  # op 13 under kind 6 stays an unknown operator
    assert re.search(r"#define\s+NQE_MAX_MATCH_PATTERN\s+4096\b", header)
    cpp = read("naive_query_engine_amd", "host", "naive_db.hpp")
    assert "struct PhysicalStringMatchExpr : PhysicalExpr" in cpp and "n.kind = NQE_EXPR_STRING_MATCH;" in cpp
    assert "enum class MatchOperator : int32_t { Like = 0, NotLike = 1, ILike = 2, NotILike = 3, StartsWith = 4, EndsWith = 5, Contains = 6, StrPos = 7 }" in cpp
    body = cpp[cpp.index("struct PhysicalStringMatchExpr"):]
    body = body[:body.index("\n};")]
    assert "n.op = int32_t(op);" in body and "MatchOperator op;" in body and body.index("expr->flatten") < body.index("pattern->flatten")
    assert "n.kind == NQE_EXPR_STRING_MATCH" in cpp  # the static-type stack walk pops two
    rust = read("integration", "rust", "gpu.rs")
    assert int(re.search(r"const NQE_EXPR_STRING_MATCH: i32 = (\d+);", rust).group(1)) == 6
    assert "pub struct PhysicalStringMatchExpr" in rust and "impl PhysicalExpr for PhysicalStringMatchExpr" in rust
    assert "kind: NQE_EXPR_STRING_MATCH, op: m.op as i32" in rust
    assert "pub enum MatchOperator { Like = 0, NotLike = 1, ILike = 2, NotILike = 3, StartsWith = 4, EndsWith = 5, Contains = 6, StrPos = 7 }" in rust
    assert "NQE_EXPR_STRING_MATCH = 6" in read("INTEGRATION.md")
    assert subprocess.run(["python", os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True).returncode == 0


def test_static_dtype_of_the_python_mirror():
    from naive_query_engine_amd import DType, Field, Operator, UnaryOperator
    from naive_query_engine_amd import expression as e
    from naive_query_engine_amd.physical_plan import _static_dtype

    col = e.col
    schema = [Field("id", DType.INT64, False), Field("s", DType.UTF8, True), Field("v", DType.FLOAT64, False)]
    for helper in (e.like, e.not_like, e.ilike, e.not_ilike, e.starts_with, e.ends_with, e.contains):
        assert _static_dtype(helper(col("s"), "a"), schema) == DType.BOOLEAN
        assert _static_dtype(helper(e.strop(UnaryOperator.Lower, col("s")), None), schema) == DType.BOOLEAN
    assert _static_dtype(e.strpos(col("s"), "-"), schema) == DType.INT64
    assert _static_dtype(e.binop(e.strpos(col("s"), "-"), Operator.Plus, e.lit_i64(1)), schema) == DType.INT64
    assert _static_dtype(e.binop(e.strpos(col("s"), "-"), Operator.Gt, e.lit_i64(0)), schema) == DType.BOOLEAN
    assert _static_dtype(e.substr(col("s"), e.strpos(col("s"), "-")), schema) == DType.UTF8
    assert _static_dtype(e.substr(col("s"), 1, 2), schema) == DType.UTF8 and _static_dtype(e.strop(UnaryOperator.CharacterLength, col("s")), schema) == DType.INT64  # what was there


def test_the_package_exports_the_node():
    import naive_query_engine_amd as pkg

    assert "PhysicalStringMatchExpr" in pkg.__all__ and "MatchOperator" in pkg.__all__ and pkg.PhysicalStringMatchExpr.create is not None
    assert "PhysicalStringExpr" in pkg.__all__ and "PhysicalStringArgsExpr" in pkg.__all__ and "PhysicalUnaryExpr" in pkg.__all__
    for name in ("like", "not_like", "ilike", "not_ilike", "starts_with", "ends_with", "contains", "strpos", "node_string_match"):
        assert callable(getattr(pkg.expression, name))
