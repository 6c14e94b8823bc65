"""CPU-only checks of PhysicalCastExpr (quirk Q29: NQE_EXPR_CAST): the flat encoding (`x CAST`: kind 8, the target in `dtype`, nothing
else set), the helper's argument checks, the static dtype of the Python mirror, the exports, the agreement of the places that spell the new
constant (include/nqe.h, arrow_host.py, host/naive_db.hpp, integration/rust/gpu.rs), and the Rust shim check."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_flatten_is_the_operand_then_the_cast_node():
    from naive_query_engine_amd import DType, Operator, PhysicalCastExpr, UnaryOperator
    from naive_query_engine_amd import expression as e
    from naive_query_engine_amd.arrow_host import EXPR_BINARY, EXPR_CAST, EXPR_COLUMN, EXPR_CONDITIONAL, EXPR_LITERAL, EXPR_STRING, node_cast
    from tests.helpers import fields

    f = fields("id", "v", "b", "s")
    assert EXPR_CAST == 8
    n = node_cast(DType.FLOAT64)
    assert (n.kind, n.op, n.column, n.dtype, n.is_null, n.utf8_length, n.value.u64) == (8, 0, 0, 4, 0, 0, 0)
    for dt in (DType.BOOLEAN, DType.INT64, DType.UINT64, DType.FLOAT64, DType.UTF8):
        nodes = e.cast(e.col("id"), dt).flatten(f)
        assert [(x.kind, x.column, x.dtype) for x in nodes] == [(EXPR_COLUMN, 0, 0), (EXPR_CAST, 0, int(dt))]
        assert [(x.kind, x.dtype) for x in PhysicalCastExpr.create(e.col("s"), dt).flatten(f)] == [(EXPR_COLUMN, 0), (EXPR_CAST, int(dt))]
    # cast(id as double) * 1.5: `id CAST 1.5 *`
    nodes = e.binop(e.cast(e.col("id"), DType.FLOAT64), Operator.Multiply, e.lit_f64(1.5)).flatten(f)
    assert [(x.kind, x.dtype) for x in nodes] == [(EXPR_COLUMN, 0), (EXPR_CAST, 4), (EXPR_LITERAL, 4), (EXPR_BINARY, 0)] and nodes[3].op == int(Operator.Multiply)
    # coalesce(v, cast(0 as double)), cast(character_length(s) as double), a cast of a cast
    nodes = e.coalesce(e.col("v"), e.cast(e.lit_i64(0), DType.FLOAT64)).flatten(f)
    assert [(x.kind, x.dtype) for x in nodes] == [(EXPR_COLUMN, 0), (EXPR_LITERAL, 2), (EXPR_CAST, 4), (EXPR_CONDITIONAL, 0)]
    nodes = e.cast(e.PhysicalStringExpr.create(e.col("s"), UnaryOperator.CharacterLength), DType.FLOAT64).flatten(f)
    assert [(x.kind, x.dtype) for x in nodes] == [(EXPR_COLUMN, 0), (EXPR_STRING, 0), (EXPR_CAST, 4)]
    nodes = e.cast(e.cast(e.col("s"), DType.FLOAT64), DType.INT64).flatten(f)
    assert [(x.kind, x.dtype) for x in nodes] == [(EXPR_COLUMN, 0), (EXPR_CAST, 4), (EXPR_CAST, 2)]
    assert e.cast(e.col("s"), DType.INT64).referenced_columns(f) == [3]
    assert repr(e.cast(e.col("id"), DType.FLOAT64)).startswith("CAST(ColumnExpr(") and repr(e.cast(e.col("id"), DType.FLOAT64)).endswith(" AS FLOAT64)")
    # the class encodes any target as it is: the library refuses it (rule 1 of include/nqe.h)
    assert [x.dtype for x in PhysicalCastExpr.create(e.col("id"), 0).flatten(f)] == [0, 0] and PhysicalCastExpr.create(e.col("id"), 77).flatten(f)[1].dtype == 77


def test_the_helper_checks_its_arguments():
    from naive_query_engine_amd import DType
    from naive_query_engine_amd import expression as e

    assert e.cast(e.col(0), 4).data_type is DType.FLOAT64 and e.cast(e.col(0), DType.UTF8).data_type is DType.UTF8
    with pytest.raises(ValueError):
        e.cast(e.col(0), DType.NULL)
    with pytest.raises(ValueError):
        e.cast(e.col(0), 6)
    with pytest.raises(ValueError):
        e.cast(e.col(0), "double")
    with pytest.raises(TypeError):
        e.cast(1.5, DType.INT64)
    with pytest.raises(TypeError):
        e.cast("id", DType.INT64)
    e.cast(e.col(0), DType.UTF8)  # Float64 -> Utf8 is the library's to refuse: the helper does not know the operand's type


def test_the_static_dtype_and_the_exports():
    import naive_query_engine_amd as nqe
    from naive_query_engine_amd import DType, Field, Operator
    from naive_query_engine_amd import expression as e
    from naive_query_engine_amd import physical_plan as pp

    assert "PhysicalCastExpr" in nqe.__all__ and nqe.PhysicalCastExpr is e.PhysicalCastExpr and issubclass(e.PhysicalCastExpr, e.PhysicalExpr)
    schema = [Field("id", DType.INT64, True), Field("s", DType.UTF8, True)]
    for dt in (DType.BOOLEAN, DType.INT64, DType.UINT64, DType.FLOAT64, DType.UTF8):
        assert pp._static_dtype(e.cast(e.col("s"), dt), schema) == dt
    assert pp._static_dtype(e.binop(e.cast(e.col("id"), DType.FLOAT64), Operator.Multiply, e.lit_f64(1.5)), schema) == DType.FLOAT64
    assert pp._static_dtype(e.coalesce(e.cast(e.col("s"), DType.INT64), e.col("id")), schema) == DType.INT64


def test_the_constant_is_spelled_the_same_everywhere():
    header = read("include", "nqe.h")
    assert re.search(r"^#define NQE_EXPR_CAST 8$", header, re.M) and "nqe_expr_cast_is_8" in header
    assert re.search(r"#define NQE_ABI_VERSION 1\b", header)
    enum = re.search(r"typedef enum nqe_expr_kind \{([^}]*)\}", header).group(1)
    assert "CAST" not in enum and "CONDITIONAL" not in enum  # the enum's list of NAME = value pairs is frozen
    assert re.search(r"^EXPR_CAST = 8\b", read("naive_query_engine_amd", "arrow_host.py"), re.M)
    hpp = read("naive_query_engine_amd", "host", "naive_db.hpp")
    assert "struct PhysicalCastExpr : PhysicalExpr" in hpp and 'static_assert(EXPR_CAST == 8' in hpp and "n.kind = NQE_EXPR_CAST;" in hpp
    rust = read("integration", "rust", "gpu.rs")
    assert "const NQE_EXPR_CAST: i32 = 8;" in rust and "downcast_ref::<PhysicalCastExpr>()" in rust and "kind: NQE_EXPR_CAST, dtype" in rust
    assert "NQE_EXPR_CAST = 8" in read("INTEGRATION.md")
    for doc, marks in [("SURVEY.md", ["| Q29 |"]), ("DESIGN.md", ["3.23", "cast_parts.hpp"]), ("README.md", ["PhysicalCastExpr", "cast.hip"])]:
        text = read(doc)
        assert all(m in text for m in marks), doc
    # the definition's error order, in the header
    flat = " ".join(header.replace("*", " ").split())  # the comment's line breaks and stars are not part of its meaning
    at = [flat.index(s) for s in ("`dtype` outside NQE_BOOLEAN..NQE_UTF8", "no operand on the stack", "an operand of dtype NQE_NULLTYPE → NQE_ERR_NOT_SUPPORTED; Float64 -> Utf8")]
    assert at == sorted(at)


def test_the_rust_shim_check_passes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_rust_shim.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok:"), out.stdout + out.stderr
