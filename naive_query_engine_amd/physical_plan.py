"""Host mirror of the reference's physical operators (src/physical_plan/*.rs).

Same class names, constructor arguments, `schema()/execute()/children()` surface and error
behaviour as the reference, so plans are written as in its tests:

    scan = ScanPlan.create(MemTable.try_create(schema, [batch]), None)
    sel  = SelectionPlan.create(scan, PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None),
                                                                Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(1))))
    batches = sel.execute()          # Vec<RecordBatch> — here: device-resident batches

`execute()` returns `DeviceRecordBatch`es (columns stay in HBM between operators; `.to_host()`
downloads).  All computation goes through the C ABI (capi → libnqe_hip.so); there is no host
fallback.  Every operator here does exactly what its reference namesake does, one operator at a
time; the fused device entry points (Projection∘Selection, Aggregate∘Selection) are introduced
by a separate pass over the tree, `rewrite()` in rewrite.py — `rewrite(tree).execute()` equals
`tree.execute()`, which tests/test_gpu_plans.py checks.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import capi
from .arrow_host import AggregateFunc, Column, DType, ErrorCode, Field, Operator, RecordBatch, ScalarValue, SetOp, Status, UnaryOperator, WindowFrame, WindowFrameEx, WindowFunc, WindowFuncEx
from .expression import ColumnExpr, CondOperator, MatchOperator, PhysicalBinaryExpr, PhysicalCastExpr, PhysicalConditionalExpr, PhysicalExpr, PhysicalLiteralExpr, PhysicalStringArgsExpr, PhysicalStringExpr, PhysicalStringMatchExpr

NaiveSchema = List[Field]  # src/logical_plan/schema.rs (qualifiers are ignored at physical planning, Q12)


def field_with_unqualified_name(schema: Sequence[Field], name: str) -> Field:
    """NaiveSchema::field_with_unqualified_name (schema.rs:116-125): first match."""
    for f in schema:
        if f.name == name:
            return f
    raise ErrorCode(Status.PlanError, f"No field named '{name}'")


class DeviceRecordBatch:
    """A RecordBatch whose columns live in HBM (nqe_table handle + field names)."""

    def __init__(self, fields: Sequence[Field], table: "capi.Table"):
        self.fields = list(fields)
        self.table = table

    @property
    def num_rows(self) -> int:
        return self.table.num_rows

    @property
    def num_columns(self) -> int:
        return self.table.num_columns

    def to_host(self) -> RecordBatch:
        cols = self.table.to_host()
        return RecordBatch([Field(f.name, c.dtype, c.validity is not None) for f, c in zip(self.fields, cols)], cols)

    def column(self, i: int) -> Column:
        return self.table.download_column(i)


# ----------------------------------------------------------------------------- data sources
class MemTable:
    """src/datasource/memory.rs:14-46 — batches are uploaded to HBM once, at creation."""

    def __init__(self, schema: NaiveSchema, batches: List[DeviceRecordBatch]):
        self._schema = list(schema)
        self.batches = batches

    @staticmethod
    def try_create(schema: NaiveSchema, batches: Sequence[RecordBatch], ctx: Optional["capi.Context"] = None) -> "MemTable":
        ctx = ctx or capi.default_context()
        dev = [DeviceRecordBatch(schema, ctx.table_from_host(b.columns)) for b in batches]
        return MemTable(schema, dev)

    @staticmethod
    def from_device(schema: NaiveSchema, tables: Sequence["capi.Table"]) -> "MemTable":
        return MemTable(schema, [DeviceRecordBatch(schema, t) for t in tables])

    def schema(self) -> NaiveSchema:
        return self._schema

    def scan(self, projection: Optional[Sequence[int]]) -> List[DeviceRecordBatch]:
        if projection is None:
            return list(self.batches)  # Arc clones (memory.rs:41)
        out = []
        for b in self.batches:  # RecordBatch::project (memory.rs:33-38)
            t = b.table.ctx.project(b.table, list(projection))
            out.append(DeviceRecordBatch([b.fields[i] for i in projection], t))
        return out

    def source_name(self) -> str:
        return "MemTable"


class CsvConfig:
    """src/datasource/csv.rs:23-43 (file_projection / datetime_format are not mirrored)"""

    def __init__(self, has_header: bool = True, delimiter: str = ",", max_read_records: Optional[int] = 3, batch_size: int = 1_000_000):
        self.has_header, self.delimiter, self.max_read_records, self.batch_size = has_header, delimiter, max_read_records, batch_size


class CsvTable(MemTable):
    """src/datasource/csv.rs:46-103 — schema inferred from the first max_read_records records, only the first batch is
    loaded (Q1); scan ignores projection (Q2).  The file image is parsed on the GPU (nqe_csv_read)."""

    @staticmethod
    def try_create(filename: str, csv_config: Optional[CsvConfig] = None, ctx: Optional["capi.Context"] = None) -> "CsvTable":
        cfg = csv_config or CsvConfig()
        ctx = ctx or capi.default_context()
        with open(filename, "rb") as f:
            data = f.read()
        mrr = -1 if cfg.max_read_records is None else cfg.max_read_records
        names, dtypes, nullable = ctx.csv_infer_schema(data, cfg.has_header, cfg.delimiter, mrr, cfg.batch_size)
        table = ctx.csv_read(data, dtypes, cfg.has_header, cfg.delimiter, cfg.batch_size)
        fields = [Field(n, d, nl) for n, d, nl in zip(names, dtypes, nullable)]
        return CsvTable(fields, [DeviceRecordBatch(fields, table)])

    def scan(self, projection):
        return list(self.batches)

    def source_name(self) -> str:
        return "CsvTable"


# ----------------------------------------------------------------------------- plans
class PhysicalPlan:
    """trait PhysicalPlan (src/physical_plan/plan.rs:14-21)."""

    def schema(self) -> NaiveSchema:
        raise NotImplementedError

    def execute(self) -> List[DeviceRecordBatch]:
        raise NotImplementedError

    def children(self) -> List["PhysicalPlan"]:
        raise NotImplementedError


class ScanPlan(PhysicalPlan):
    """src/physical_plan/scan.rs:18-41"""

    def __init__(self, source, projection):
        self.source, self.projection = source, projection

    @staticmethod
    def create(source, projection: Optional[Sequence[int]] = None) -> "ScanPlan":
        return ScanPlan(source, projection)

    def schema(self):
        return self.source.schema()

    def execute(self):
        return self.source.scan(self.projection)

    def children(self):
        return []


def _ctx_of(batches: Sequence[DeviceRecordBatch]) -> "capi.Context":
    return batches[0].table.ctx if batches else capi.default_context()


def _one_table(ctx, batches):
    return batches[0].table if len(batches) == 1 else ctx.concat([b.table for b in batches])


class _KeyedTable:
    """The batches as one table whose key and argument expressions are column indices (run_window_plan's first half in the C++ mirror):
    a bare ColumnExpr is its index, any other expression is evaluated into a temporary column behind the input's."""

    def __init__(self, ctx, batches, fields):
        self.ctx, self.fields, self.table, self.temps = ctx, fields, _one_table(ctx, batches), []

    def column_of(self, expr: PhysicalExpr) -> int:
        if isinstance(expr, ColumnExpr):
            return expr.resolve(self.fields)
        self.temps.append(self.ctx.expr_evaluate(self.table, expr.flatten(self.fields)))
        return len(self.fields) + len(self.temps) - 1

    def source(self):
        """the table an operator reads: the input itself when no temporary was made"""
        return self.ctx.append_columns(self.table, self.temps) if self.temps else self.table

    def without_temps(self, out):
        """an output with source()'s columns, the temporaries projected away"""
        return self.ctx.project(out, list(range(len(self.fields)))) if self.temps else out


class SelectionPlan(PhysicalPlan):
    """src/physical_plan/selection.rs:23-112"""

    def __init__(self, input: PhysicalPlan, expr: PhysicalExpr):
        self.input, self.expr = input, expr

    @staticmethod
    def create(input: PhysicalPlan, expr: PhysicalExpr) -> "SelectionPlan":
        return SelectionPlan(input, expr)

    def schema(self):
        return self.input.schema()

    def execute(self):
        batches = self.input.execute()
        if not batches:  # input[0] panics (selection.rs:60)
            raise ErrorCode(Status.NotSupported, "index out of bounds: input[0] (selection.rs:60 panics)")
        ctx = _ctx_of(batches)
        pred = self.expr.flatten(batches[0].fields)
        if len(batches) == 1:
            return [DeviceRecordBatch(batches[0].fields, ctx.selection(batches[0].table, pred))]
        # quirk Q3: the predicate is evaluated on batch 0 only and zipped against every batch
        mask = ctx.expr_evaluate(batches[0].table, pred)
        return [DeviceRecordBatch(b.fields, ctx.filter(b.table, mask, 0)) for b in batches]

    def children(self):
        return [self.input]


class ProjectionPlan(PhysicalPlan):
    """src/physical_plan/projection.rs:18-75"""

    def __init__(self, input: PhysicalPlan, schema: NaiveSchema, expr: Sequence[PhysicalExpr]):
        self.input, self._schema, self.expr = input, list(schema), list(expr)

    @staticmethod
    def create(input: PhysicalPlan, schema: NaiveSchema, expr: Sequence[PhysicalExpr]) -> "ProjectionPlan":
        return ProjectionPlan(input, schema, expr)

    def schema(self):
        return self._schema

    def _out_fields(self, cols_dtypes):
        return [Field(f.name, dt, True) for f, dt in zip(self._schema, cols_dtypes)]

    def execute(self):
        if not self._schema:  # projection.rs:47-48: pass-through above an aggregate
            return self.input.execute()
        batches = self.input.execute()
        out = []
        for b in batches:
            ctx = b.table.ctx
            t = ctx.projection(b.table, [e.flatten(b.fields) for e in self.expr])
            out.append(DeviceRecordBatch(self._out_fields(t.dtypes()), t))
        return out

    def children(self):
        return [self.input]


class _Materialized(PhysicalPlan):
    """already-executed child (avoids executing a subtree twice when a fusion attempt falls through)"""

    def __init__(self, batches, schema):
        self._batches, self._schema = batches, schema

    def schema(self):
        return self._schema

    def execute(self):
        return self._batches

    def children(self):
        return []


class PhysicalLimitPlan(PhysicalPlan):
    """src/physical_plan/limit.rs:32-49"""

    def __init__(self, input, n):
        self.input, self.n = input, n

    @staticmethod
    def create(input, n: int):
        return PhysicalLimitPlan(input, n)

    def schema(self):
        return self.input.schema()

    def execute(self):
        n, ret = self.n, []
        for b in self.input.execute():
            if n == 0:
                break
            if b.num_rows <= n:
                ret.append(b)
                n -= b.num_rows
            else:
                ret.append(DeviceRecordBatch(b.fields, b.table.ctx.slice(b.table, 0, n)))
                n = 0
        return ret

    def children(self):
        return [self.input]


class PhysicalOffsetPlan(PhysicalPlan):
    """src/physical_plan/offset.rs:30-51"""

    def __init__(self, input, n):
        self.input, self.n = input, n

    @staticmethod
    def create(input, n: int):
        return PhysicalOffsetPlan(input, n)

    def schema(self):
        return self.input.schema()

    def execute(self):
        n, ret = self.n, []
        for b in self.input.execute():
            if n == 0:
                ret.append(b)
                continue
            if n >= b.num_rows:
                n -= b.num_rows
                continue
            ret.append(DeviceRecordBatch(b.fields, b.table.ctx.slice(b.table, n, b.num_rows - n)))
            n = 0
        return ret

    def children(self):
        return [self.input]


# ----------------------------------------------------------------------------- aggregates
class AggregateOperator:
    """trait AggregateOperator (src/physical_plan/aggregate/mod.rs:225-235).  The per-row
    update()/update_batch() loops run on the device; the host object only names the function,
    its column and the output field."""

    func: AggregateFunc = AggregateFunc.Count
    label = "count"
    out_dtype = DType.FLOAT64

    def __init__(self, col_expr: ColumnExpr):
        self.col_expr = col_expr

    @classmethod
    def create(cls, col_expr: ColumnExpr):
        return cls(col_expr)

    def data_field(self, schema: NaiveSchema) -> Field:
        if self.col_expr.name is not None:
            f = field_with_unqualified_name(schema, self.col_expr.name)
            return Field(f"{self.label}({f.name})", self.out_dtype, False)
        if self.col_expr.idx is not None:
            return Field(f"{self.label}({schema[self.col_expr.idx].name})", self.out_dtype, False)
        raise ErrorCode(Status.LogicalError, "ColumnExpr must has name or idx")


class Sum(AggregateOperator):
    """src/physical_plan/aggregate/sum.rs"""
    func, label = AggregateFunc.Sum, "sum"


class Avg(AggregateOperator):
    """src/physical_plan/aggregate/avg.rs"""
    func, label = AggregateFunc.Avg, "avg"


class Count(AggregateOperator):
    """src/physical_plan/aggregate/count.rs"""
    func, label, out_dtype = AggregateFunc.Count, "count", DType.UINT64


class Max(AggregateOperator):
    """src/physical_plan/aggregate/max.rs"""
    func, label = AggregateFunc.Max, "max"


class Min(AggregateOperator):
    """src/physical_plan/aggregate/min.rs"""
    func, label = AggregateFunc.Min, "min"


class PhysicalAggregatePlan(PhysicalPlan):
    """src/physical_plan/aggregate/mod.rs:31-223"""

    def __init__(self, group_expr, aggr_ops, input):
        self.group_expr, self.aggr_ops, self.input = list(group_expr), list(aggr_ops), input
        self._schema = list(input.schema())
        self._ungrouped_state = None  # quirk Q9: un-grouped state is never cleared between execute() calls

    @staticmethod
    def create(group_expr: Sequence[PhysicalExpr], aggr_ops: Sequence[AggregateOperator], input: PhysicalPlan):
        return PhysicalAggregatePlan(group_expr, aggr_ops, input)

    def schema(self):
        return self._schema  # the INPUT schema (quirk Q8/Q13)

    def children(self):
        return [self.input]

    def _input_batches(self):
        """(input batches, predicate expression the aggregation kernel applies itself): the plain operator has no predicate"""
        return self.input.execute(), None

    def execute(self):
        out_fields = [op.data_field(self._schema) for op in self.aggr_ops]
        batches, pred_expr = self._input_batches()
        ctx = _ctx_of(batches)
        if not batches:
            if self.group_expr:
                # concat_batches of an empty Vec → empty batch → zero groups
                raise ErrorCode(Status.NotSupported, "aggregate over an empty batch list is not supported on the device path")
            raise ErrorCode(Status.NotSupported, "aggregate over an empty batch list is not supported on the device path")
        fields = batches[0].fields
        aggs = [(op.func, op.col_expr.resolve(fields)) for op in self.aggr_ops]
        pred = pred_expr.flatten(fields) if pred_expr is not None else None
        if not self.group_expr:
            # update_batch per batch (:123-139): partial state per batch, merged with the running state
            parts = [ctx.aggregate_partial(b.table, aggs, pred_nodes=pred)[0] for b in batches]
            if self._ungrouped_state is not None:
                parts.insert(0, self._ungrouped_state)
            if len(parts) > 1 or self._ungrouped_state is not None:
                # keep the merged raw state for the next execute() (Q9)
                merged_state = _merge_raw_state(ctx, parts, aggs)
            else:
                merged_state = parts[0]
            self._ungrouped_state = merged_state
            out, _ = ctx.aggregate_merge([merged_state], None, aggs)
            return [DeviceRecordBatch(out_fields, out)]
        # grouped: concat_batches, then group by group_expr[0] only (:143-148)
        table = _one_table(ctx, batches)
        key = self.group_expr[0].flatten(fields)
        out = ctx.aggregate(table, aggs, group_nodes=key, pred_nodes=pred)
        return [DeviceRecordBatch(out_fields, out)]


class GroupedAggregatePlan(PhysicalPlan):
    """GROUP BY honouring EVERY group expression (quirk Q20; PhysicalAggregatePlan above keeps the reference's group_expr[0], Q8).  The
    input batches are concatenated and ONE batch leaves: the key columns in key order, then one column per aggregate (Q13's logical
    order), sorted ascending by the key tuple.  A row with a NULL in any key is dropped.  A key field takes the column's field name
    for a bare ColumnExpr and `group_<i>` otherwise.  Nothing is kept between execute() calls."""

    def __init__(self, group_expr, aggr_ops, input):
        self.group_expr, self.aggr_ops, self.input = list(group_expr), list(aggr_ops), input
        if not self.group_expr:
            raise ErrorCode(Status.PlanError, "GroupedAggregatePlan: the list of group expressions is empty (the un-grouped form is PhysicalAggregatePlan's)")

    @staticmethod
    def create(group_expr: Sequence[PhysicalExpr], aggr_ops: Sequence[AggregateOperator], input: PhysicalPlan) -> "GroupedAggregatePlan":
        return GroupedAggregatePlan(group_expr, aggr_ops, input)

    def _key_fields(self, fields: Sequence[Field], dtypes=None) -> List[Field]:
        out = []
        for i, e in enumerate(self.group_expr):
            cols = e.referenced_columns(fields)
            name = fields[cols[0]].name if isinstance(e, ColumnExpr) else f"group_{i}"
            # (before execution: integer arithmetic keeps its operands' type, so the first referenced column's type stands in)
            dt = dtypes[i] if dtypes is not None else (fields[cols[0]].dtype if cols else DType.INT64)
            out.append(Field(name, dt, False))
        return out

    def schema(self):
        below = list(self.input.schema())
        return self._key_fields(below) + [op.data_field(below) for op in self.aggr_ops]

    def children(self):
        return [self.input]

    def _input_batches(self):
        """(input batches, predicate expression the operator applies itself): the plain operator has no predicate"""
        return self.input.execute(), None

    def execute(self):
        batches, pred_expr = self._input_batches()
        if not batches:
            raise ErrorCode(Status.NotSupported, "aggregate over an empty batch list is not supported on the device path")
        ctx = _ctx_of(batches)
        fields = batches[0].fields
        table = _one_table(ctx, batches)
        aggs = [(op.func, op.col_expr.resolve(fields)) for op in self.aggr_ops]
        pred = pred_expr.flatten(fields) if pred_expr is not None else None
        out = ctx.group_aggregate(table, [e.flatten(fields) for e in self.group_expr], aggs, pred_nodes=pred)
        k = len(self.group_expr)
        out_fields = self._key_fields(fields, out.dtypes()[:k]) + [op.data_field(fields) for op in self.aggr_ops]
        return [DeviceRecordBatch(out_fields, out)]


def _merge_raw_state(ctx, parts, aggs):
    """Un-grouped raw states are single rows of (count,sum,min,max) per aggregate and the merge is
    associative, so the running state is simply the concatenation of the partial rows; it is folded
    by nqe_aggregate_merge whenever a result is needed."""
    return ctx.concat(parts)


# ----------------------------------------------------------------------------- hash join
@dataclass(frozen=True)
class ColumnRef:
    """logical_plan::expression::Column (expression.rs:167-170)"""

    table: Optional[str]
    name: str


class JoinType:
    Inner, Left, Right, Cross = range(4)


class HashJoin(PhysicalPlan):
    """src/physical_plan/hash_join.rs:44-289 — LEFT child = build side, RIGHT = probe side (Q11)."""

    def __init__(self, left, right, on, join_type, schema):
        self.left, self.right, self.on, self.join_type, self._schema = left, right, list(on), join_type, list(schema)
        self._executions = 0  # the reference never clears its hash table between execute() calls (quirk Q11)

    @staticmethod
    def create(left: PhysicalPlan, right: PhysicalPlan, on: Sequence[Tuple[ColumnRef, ColumnRef]], join_type, schema: NaiveSchema):
        return HashJoin(left, right, on, join_type, schema)

    def schema(self):
        return self._schema

    def children(self):
        return [self.left, self.right]

    def execute(self):
        if not self.on:  # hash_join.rs:125-129
            raise ErrorCode(Status.PlanError, "Inner Join on Conditions can't not be empty")
        lb = self.left.execute()
        rb = self.right.execute()
        ctx = _ctx_of(lb or rb)
        if not lb:
            raise ErrorCode(Status.NotSupported, "join with an empty left batch list is not supported on the device path")
        ltab = _one_table(ctx, lb)  # concat_batches (:132)
        lkey = ColumnExpr.try_create(self.on[0][0].name, None).resolve(lb[0].fields)  # by NAME, first match (:134-136)
        # Q11: build() pushes the row indices into the SAME map again on every execute(), so the k-th execute() emits each
        # match k times, in the order [matches of the first build..., of the second...].  A build side of k copies of the
        # left batch has exactly that match order (row i + c*n carries the payload of row i).
        self._executions += 1
        if self._executions > 1:
            ltab = ctx.concat([ltab] * self._executions)
        jt = ctx.hash_join_build(ltab, lkey)
        out = []
        for b in rb:  # one output batch per probe batch (:177-250)
            rkey = ColumnExpr.try_create(self.on[0][1].name, None).resolve(b.fields)
            t = ctx.hash_join_probe(jt, b.table, rkey)
            fields = self._schema if len(self._schema) == t.num_columns else list(lb[0].fields) + list(b.fields)
            out.append(DeviceRecordBatch(fields, t))
        return out


# ----------------------------------------------------------------------------- outer hash join
class HashOuterJoin(PhysicalPlan):
    """HashJoin honouring `join_type` (quirk Q19; the reference's HashJoin stores the type and never reads it).  The match relation
    is HashJoin's, Q11 included: LEFT child = build side, RIGHT = probe side, only on[0], key validity ignored.  Inner: the inner
    join.  Right: one output batch per probe batch; a probe row without a match emits one row with every left column NULL.  Left:
    the probe batches' outputs are the inner join's, and one final batch — always emitted, possibly with 0 rows — holds the build
    rows that matched in no probe batch, in ascending build row, with every right column NULL.  Cross raises PlanError.  Nothing
    is kept between execute() calls (no Q11 re-execution duplication)."""

    def __init__(self, left, right, on, join_type, schema):
        self.left, self.right, self.on, self.join_type, self._schema = left, right, list(on), join_type, list(schema)

    @staticmethod
    def create(left: PhysicalPlan, right: PhysicalPlan, on: Sequence[Tuple[ColumnRef, ColumnRef]], join_type, schema: NaiveSchema) -> "HashOuterJoin":
        return HashOuterJoin(left, right, on, join_type, schema)

    def schema(self):
        return self._schema

    def children(self):
        return [self.left, self.right]

    def execute(self):
        if not self.on:  # as HashJoin (hash_join.rs:125-129)
            raise ErrorCode(Status.PlanError, "Inner Join on Conditions can't not be empty")
        if self.join_type not in (JoinType.Inner, JoinType.Left, JoinType.Right):
            raise ErrorCode(Status.PlanError, "HashOuterJoin: the join type must be Inner, Left or Right")
        lb = self.left.execute()
        rb = self.right.execute()
        ctx = _ctx_of(lb or rb)
        if not lb:
            raise ErrorCode(Status.NotSupported, "join with an empty left batch list is not supported on the device path")
        ltab = _one_table(ctx, lb)  # concat_batches (:132)
        lkey = ColumnExpr.try_create(self.on[0][0].name, None).resolve(lb[0].fields)  # by NAME, first match (:134-136)
        jt = ctx.hash_join_build(ltab, lkey)
        marks = ctx.join_marks(jt) if self.join_type == JoinType.Left else None
        ncols = len(lb[0].fields) + len(self.right.schema())
        out = []
        for b in rb:  # one output batch per probe batch
            rkey = ColumnExpr.try_create(self.on[0][1].name, None).resolve(b.fields)
            if self.join_type == JoinType.Inner:
                t = ctx.hash_join_probe(jt, b.table, rkey)
            else:
                t = ctx.hash_join_probe_outer(jt, b.table, rkey, keep_probe=self.join_type == JoinType.Right, marks=marks)
            fields = self._schema if len(self._schema) == t.num_columns else list(lb[0].fields) + list(b.fields)
            out.append(DeviceRecordBatch(fields, t))
        if self.join_type == JoinType.Left:  # the build rows no probe batch matched; dtypes from the probe child's schema
            rfields = list(rb[0].fields) if rb else list(self.right.schema())
            t = ctx.hash_join_unmatched_build(jt, marks, [f.dtype for f in rfields])
            fields = self._schema if len(self._schema) == ncols else list(lb[0].fields) + rfields
            out.append(DeviceRecordBatch(fields, t))
        return out


# ----------------------------------------------------------------------------- hash join on several keys
class MultiKeyHashJoin(PhysicalPlan):
    """HashJoin honouring every `on` pair (quirk Q21; the reference's HashJoin reads on[0] alone) and `join_type` as HashOuterJoin
    does.  The match relation is HashJoin's, Q11 included, applied to every pair: LEFT child = build side, RIGHT = probe side, key
    validity ignored at every position.  Every pair is resolved by NAME, first match (Q12): the left names against the first left
    batch, the right names per probe batch.  Batches, row order and NULL-extension are HashOuterJoin's; with one pair its batches
    equal HashOuterJoin's.  Cross raises PlanError; an empty `on` raises PlanError after both children ran.  Nothing is kept between
    execute() calls (no Q11 re-execution duplication)."""

    def __init__(self, left, right, on, join_type, schema):
        self.left, self.right, self.on, self.join_type, self._schema = left, right, list(on), join_type, list(schema)

    @staticmethod
    def create(left: PhysicalPlan, right: PhysicalPlan, on: Sequence[Tuple[ColumnRef, ColumnRef]], join_type, schema: NaiveSchema) -> "MultiKeyHashJoin":
        return MultiKeyHashJoin(left, right, on, join_type, schema)

    def schema(self):
        return self._schema

    def children(self):
        return [self.left, self.right]

    def execute(self):
        if self.join_type not in (JoinType.Inner, JoinType.Left, JoinType.Right):
            raise ErrorCode(Status.PlanError, "MultiKeyHashJoin: the join type must be Inner, Left or Right")
        lb = self.left.execute()
        rb = self.right.execute()
        if not self.on:  # as HashJoin (hash_join.rs:125-129)
            raise ErrorCode(Status.PlanError, "Inner Join on Conditions can't not be empty")
        ctx = _ctx_of(lb or rb)
        if not lb:
            raise ErrorCode(Status.NotSupported, "join with an empty left batch list is not supported on the device path")
        ltab = _one_table(ctx, lb)  # concat_batches (:132)
        lkeys = [ColumnExpr.try_create(l.name, None).resolve(lb[0].fields) for l, _ in self.on]  # by NAME, first match (:134-136)
        jt = ctx.hash_join_build_keys(ltab, lkeys)
        marks = ctx.join_marks(jt) if self.join_type == JoinType.Left else None
        ncols = len(lb[0].fields) + len(self.right.schema())
        out = []
        for b in rb:  # one output batch per probe batch
            rkeys = [ColumnExpr.try_create(r.name, None).resolve(b.fields) for _, r in self.on]
            t = ctx.hash_join_probe_keys(jt, b.table, rkeys, keep_probe=self.join_type == JoinType.Right, marks=marks)
            fields = self._schema if len(self._schema) == t.num_columns else list(lb[0].fields) + list(b.fields)
            out.append(DeviceRecordBatch(fields, t))
        if self.join_type == JoinType.Left:  # the build rows no probe batch matched; dtypes from the probe child's schema
            rfields = list(rb[0].fields) if rb else list(self.right.schema())
            t = ctx.hash_join_unmatched_build(jt, marks, [f.dtype for f in rfields])
            fields = self._schema if len(self._schema) == ncols else list(lb[0].fields) + rfields
            out.append(DeviceRecordBatch(fields, t))
        return out


# ----------------------------------------------------------------------------- semi and anti hash joins
class SemiJoinType:
    ProbeSemi, ProbeAnti, BuildSemi, BuildAnti = range(4)


class HashSemiJoin(PhysicalPlan):
    """Which rows of one child have a partner in the other (quirk Q22; the reference has no such operator): the join behind
    WHERE k IN (SELECT ...), EXISTS and NOT EXISTS.  The match relation is MultiKeyHashJoin's, Q11 included: LEFT child = build side,
    RIGHT = probe side, every `on` pair resolved by NAME, first match (Q12), key validity ignored at every position — unless
    `null_key_unmatched`: then a probe row with a NULL at any key position matches nothing (a build key column with NULLs is
    NotSupported).  ProbeSemi / ProbeAnti: one output batch per probe batch with the right columns alone — the probe rows that have
    a match / have none, each once, in probe order.  BuildSemi / BuildAnti: one final batch, always emitted, possibly with 0 rows, of
    the left columns alone — the build rows that matched in some probe batch / in none, in ascending build row.  schema() is the kept
    side's schema.  An empty `on` raises PlanError after both children ran.  Nothing is kept between execute() calls."""

    def __init__(self, left, right, on, semi_type, schema, null_key_unmatched=False):
        self.left, self.right, self.on, self.semi_type, self._schema = left, right, list(on), semi_type, list(schema)
        self.null_key_unmatched = bool(null_key_unmatched)

    @staticmethod
    def create(left: PhysicalPlan, right: PhysicalPlan, on: Sequence[Tuple[ColumnRef, ColumnRef]], semi_type, schema: NaiveSchema,
               null_key_unmatched: bool = False) -> "HashSemiJoin":
        return HashSemiJoin(left, right, on, semi_type, schema, null_key_unmatched)

    def schema(self):
        return self._schema

    def children(self):
        return [self.left, self.right]

    def execute(self):
        if self.semi_type not in (SemiJoinType.ProbeSemi, SemiJoinType.ProbeAnti, SemiJoinType.BuildSemi, SemiJoinType.BuildAnti):
            raise ErrorCode(Status.PlanError, "HashSemiJoin: the semi join type must be ProbeSemi, ProbeAnti, BuildSemi or BuildAnti")
        lb = self.left.execute()
        rb = self.right.execute()
        if not self.on:  # as HashJoin (hash_join.rs:125-129)
            raise ErrorCode(Status.PlanError, "Inner Join on Conditions can't not be empty")
        ctx = _ctx_of(lb or rb)
        if not lb:
            raise ErrorCode(Status.NotSupported, "join with an empty left batch list is not supported on the device path")
        ltab = _one_table(ctx, lb)  # concat_batches (:132)
        lkeys = [ColumnExpr.try_create(l.name, None).resolve(lb[0].fields) for l, _ in self.on]  # by NAME, first match (:134-136)
        jt = ctx.hash_join_build_keys(ltab, lkeys)
        build_side = self.semi_type in (SemiJoinType.BuildSemi, SemiJoinType.BuildAnti)
        anti = self.semi_type in (SemiJoinType.ProbeAnti, SemiJoinType.BuildAnti)
        marks = ctx.join_marks(jt) if build_side else None
        out = []
        for b in rb:
            rkeys = [ColumnExpr.try_create(r.name, None).resolve(b.fields) for _, r in self.on]
            if build_side:  # the mark-only pass: no output batch
                ctx.hash_join_probe_semi(jt, b.table, rkeys, null_key_unmatched=self.null_key_unmatched, marks=marks, want_out=False)
                continue
            t = ctx.hash_join_probe_semi(jt, b.table, rkeys, anti=anti, null_key_unmatched=self.null_key_unmatched)
            out.append(DeviceRecordBatch(self._schema if len(self._schema) == t.num_columns else list(b.fields), t))
        if build_side:
            t = ctx.hash_join_marked_build(jt, marks, anti=anti)
            out.append(DeviceRecordBatch(self._schema if len(self._schema) == t.num_columns else list(lb[0].fields), t))
        return out


# ----------------------------------------------------------------------------- cross join
class CrossJoin(PhysicalPlan):
    """src/physical_plan/cross_join.rs:26-192 — one output batch per (outer, inner) batch pair, outer-major; quirk Q15: with L and R
    the pair's row counts, output row j takes left row j % L and right row j % R (a Cartesian product only when gcd(L, R) = 1), and
    no output column has a validity bitmap.  `join_type` is stored and never read; nothing is kept between execute() calls."""

    def __init__(self, left, right, join_type, schema):
        self.left, self.right, self.join_type, self._schema = left, right, join_type, list(schema)

    @staticmethod
    def create(left: PhysicalPlan, right: PhysicalPlan, join_type, schema: NaiveSchema) -> "CrossJoin":
        return CrossJoin(left, right, join_type, schema)

    def schema(self):
        return self._schema

    def children(self):
        return [self.left, self.right]

    def execute(self):
        outer = self.left.execute()
        inner = self.right.execute()
        out = []
        for o in outer:  # cross_join.rs:63-64
            for i in inner:
                t = o.table.ctx.cross_join(o.table, i.table)
                fields = self._schema if len(self._schema) == t.num_columns else list(o.fields) + list(i.fields)
                out.append(DeviceRecordBatch(fields, t))
        return out


# ----------------------------------------------------------------------------- nested loop join
class NestedLoopJoin(PhysicalPlan):
    """src/physical_plan/nested_loop_join.rs:30-184 — inner equi-join on `on[0]`, one output batch per (outer, inner) batch pair,
    outer-major (quirk Q17): NULL keys match nothing, Float64 keys are joined with IEEE ==, rows come out by ascending (left row,
    right row), payload validity is preserved.  `join_type` is stored and never read; nothing is kept between execute() calls."""

    def __init__(self, left, right, on, join_type, schema):
        self.left, self.right, self.on, self.join_type, self._schema = left, right, list(on), join_type, list(schema)

    @staticmethod
    def create(left: PhysicalPlan, right: PhysicalPlan, on: Sequence[Tuple[ColumnRef, ColumnRef]], join_type, schema: NaiveSchema) -> "NestedLoopJoin":
        return NestedLoopJoin(left, right, on, join_type, schema)

    def schema(self):
        return self._schema

    def children(self):
        return [self.left, self.right]

    def execute(self):
        outer = self.left.execute()
        inner = self.right.execute()
        if not self.on:  # after the children (:99-103): a child's error wins
            raise ErrorCode(Status.PlanError, "Inner Join on Conditions can't not be empty")
        lcol = ColumnExpr.try_create(self.on[0][0].name, None)  # only on[0] (:105), by NAME, first match
        rcol = ColumnExpr.try_create(self.on[0][1].name, None)
        out = []
        for o in outer:
            lkey = lcol.resolve(o.fields)  # in the outer loop (:111): a missing left column raises without inner batches
            for i in inner:
                rkey = rcol.resolve(i.fields)
                t = o.table.ctx.nested_loop_join(o.table, i.table, lkey, rkey)
                fields = self._schema if len(self._schema) == t.num_columns else list(o.fields) + list(i.fields)
                out.append(DeviceRecordBatch(fields, t))
        return out


# ----------------------------------------------------------------------------- order by
class PhysicalSortExpr:
    """one ORDER BY key: an expression with arrow-rs' SortOptions (default: ascending, nulls first)"""

    def __init__(self, expr: PhysicalExpr, descending: bool = False, nulls_first: bool = True):
        self.expr, self.descending, self.nulls_first = expr, bool(descending), bool(nulls_first)

    @staticmethod
    def create(expr: PhysicalExpr, descending: bool = False, nulls_first: bool = True) -> "PhysicalSortExpr":
        return PhysicalSortExpr(expr, descending, nulls_first)

    def __repr__(self):
        return f"PhysicalSortExpr({self.expr!r}, descending={self.descending}, nulls_first={self.nulls_first})"


class PhysicalSortPlan(PhysicalPlan):
    """ORDER BY (quirk Q18; the reference drops the clause, sql/planner.rs:159-162): what lexsort_to_indices + take give.  The input
    batches are concatenated (global order needs one output, as HashJoin::build's concat_batches) and ONE batch with the input's
    schema leaves: a stable sort by `sort_exprs`, first key most significant, cut to `fetch` rows when given.  A key that is a bare
    ColumnExpr is passed by index; any other expression is evaluated into a temporary column that the output drops again."""

    def __init__(self, input: PhysicalPlan, sort_exprs: Sequence[PhysicalSortExpr], fetch: Optional[int] = None):
        self.input, self.sort_exprs, self.fetch = input, list(sort_exprs), fetch

    @staticmethod
    def create(input: PhysicalPlan, sort_exprs: Sequence[PhysicalSortExpr], fetch: Optional[int] = None) -> "PhysicalSortPlan":
        return PhysicalSortPlan(input, sort_exprs, fetch)

    def schema(self):
        return self.input.schema()

    def children(self):
        return [self.input]

    def execute(self):
        batches = self.input.execute()
        if not batches:
            raise ErrorCode(Status.NotSupported, "order by over an empty batch list is not supported on the device path")
        ctx = _ctx_of(batches)
        fields = batches[0].fields
        kt = _KeyedTable(ctx, batches, fields)
        keys = [(kt.column_of(e.expr), e.descending, e.nulls_first) for e in self.sort_exprs]
        return [DeviceRecordBatch(fields, kt.without_temps(ctx.order_by(kt.source(), keys, self.fetch)))]


# ----------------------------------------------------------------------------- window functions
class WindowFunction:
    """one function of a window: ROW_NUMBER / RANK / DENSE_RANK (no argument, no frame) or one of Q10's count / sum / min / max / avg
    over `expr` and the rows of `frame` (default: RANGE ... CURRENT ROW, SQL's default with ORDER BY)"""

    def __init__(self, func: WindowFunc, expr: Optional[PhysicalExpr] = None, frame: WindowFrame = WindowFrame.Range):
        self.func, self.expr, self.frame = WindowFunc(func), expr, WindowFrame(frame)
        self._wide()  # (refuses a missing argument)

    def _wide(self) -> "WindowFunctionEx":
        """the same function of the wider entry (the enum values are equal): its argument check and its field are this one's"""
        return WindowFunctionEx(int(self.func), self.expr, int(self.frame))

    @staticmethod
    def create(func: WindowFunc, expr: Optional[PhysicalExpr] = None, frame: WindowFrame = WindowFrame.Range) -> "WindowFunction":
        return WindowFunction(func, expr, frame)

    def data_field(self, schema: NaiveSchema) -> Field:
        return self._wide().data_field(schema)

    def spec(self, column: Optional[int]) -> tuple:
        """the function as Context.window takes it"""
        return (self.func, column, self.frame)

    def __repr__(self):
        return f"WindowFunction({self.func.name}, {self.expr!r}, {self.frame.name})"


class _WindowPlan(PhysicalPlan):
    """what the two window plans share: everything but the Context method `_entry` and the function type, whose spec() that method takes"""

    _entry: str
    _fields_first = False  # whether a function's field can be refused, which then happens before anything runs

    def __init__(self, input: PhysicalPlan, partition_by: Sequence[PhysicalExpr], order_by: Sequence[PhysicalSortExpr], funcs: Sequence):
        self.input, self.partition_by, self.order_by, self.funcs = input, list(partition_by), list(order_by), list(funcs)

    @classmethod
    def create(cls, input: PhysicalPlan, partition_by: Sequence[PhysicalExpr], order_by: Sequence[PhysicalSortExpr], funcs: Sequence):
        return cls(input, partition_by, order_by, funcs)

    def schema(self):
        s = list(self.input.schema())
        return s + [f.data_field(s) for f in self.funcs]

    def children(self):
        return [self.input]

    def execute(self):
        batches = self.input.execute()
        if not batches:
            raise ErrorCode(Status.NotSupported, "window functions over an empty batch list are not supported on the device path")
        ctx = _ctx_of(batches)
        fields = batches[0].fields
        out_fields = list(fields) + [f.data_field(fields) for f in self.funcs] if self._fields_first else None
        kt = _KeyedTable(ctx, batches, fields)
        parts = [kt.column_of(e) for e in self.partition_by]
        keys = [(kt.column_of(e.expr), e.descending, e.nulls_first) for e in self.order_by]
        specs = [f.spec(None if f.expr is None else kt.column_of(f.expr)) for f in self.funcs]
        out = getattr(ctx, self._entry)(kt.source(), parts, keys, specs)
        out_fields = out_fields or list(fields) + [f.data_field(fields) for f in self.funcs]
        return [DeviceRecordBatch(out_fields, ctx.append_columns(kt.table, [ctx.project(out, [i]) for i in range(len(self.funcs))]))]


class PhysicalWindowPlan(_WindowPlan):
    """f(...) OVER (PARTITION BY partition_by ORDER BY order_by) for every WindowFunction of `funcs`, through nqe_window_execute (quirk
    Q23; the reference has no window expression, logical_plan/expression.rs:22-46): all functions share the one window.  Like
    PhysicalSortPlan the input batches are concatenated and ONE batch leaves: the input's columns in input order, then one column per
    function.  A key or argument that is a bare ColumnExpr is passed by index; any other expression is evaluated into a temporary
    column that never reaches the output."""

    _entry = "window"


# ----------------------------------------------------------------------------- window functions, the wider entry
_WINDOW_EX_LABELS = {WindowFuncEx.RowNumber: "row_number", WindowFuncEx.Rank: "rank", WindowFuncEx.DenseRank: "dense_rank", WindowFuncEx.Count: "count", WindowFuncEx.Sum: "sum",
                     WindowFuncEx.Min: "min", WindowFuncEx.Max: "max", WindowFuncEx.Avg: "avg", WindowFuncEx.Lag: "lag", WindowFuncEx.Lead: "lead",
                     WindowFuncEx.FirstValue: "first_value", WindowFuncEx.LastValue: "last_value", WindowFuncEx.Ntile: "ntile"}
_WINDOW_EX_NO_ARG = (WindowFuncEx.RowNumber, WindowFuncEx.Rank, WindowFuncEx.DenseRank, WindowFuncEx.Ntile)
_WINDOW_EX_VALUE = (WindowFuncEx.Lag, WindowFuncEx.Lead, WindowFuncEx.FirstValue, WindowFuncEx.LastValue)
_COMPARISONS = (Operator.Eq, Operator.NotEq, Operator.Lt, Operator.LtEq, Operator.Gt, Operator.GtEq, Operator.And, Operator.Or)


def _static_dtype(expr: PhysicalExpr, schema: NaiveSchema) -> DType:
    """the dtype an expression evaluates to (Q6: no coercion, so an arithmetic node has its left operand's; a unary function Float64; a string
    function Utf8, CharacterLength Int64; substr / repeat / replace Utf8; a string match Boolean, strpos Int64;
    Not / IsNull / IsNotNull Boolean, Coalesce / NullIf their first operand's, If its `then` operand's; a cast its target)"""
    if isinstance(expr, PhysicalCastExpr):
        return DType(expr.data_type)
    if isinstance(expr, PhysicalConditionalExpr):
        return DType.BOOLEAN if expr.op in (CondOperator.Not, CondOperator.IsNull, CondOperator.IsNotNull) else _static_dtype(expr.operands[1 if expr.op == CondOperator.If else 0], schema)
    if isinstance(expr, PhysicalStringMatchExpr):
        return DType.INT64 if expr.op == MatchOperator.StrPos else DType.BOOLEAN
    if isinstance(expr, PhysicalStringArgsExpr):
        return DType.UTF8
    if isinstance(expr, PhysicalStringExpr):
        return DType.INT64 if expr.func == UnaryOperator.CharacterLength else DType.UTF8
    if isinstance(expr, ColumnExpr):
        return schema[expr.resolve(schema)].dtype
    if isinstance(expr, PhysicalLiteralExpr):
        return expr.literal.dtype
    if isinstance(expr, PhysicalBinaryExpr):
        return DType.BOOLEAN if expr.op in _COMPARISONS else _static_dtype(expr.left, schema)
    return DType.FLOAT64


class WindowFunctionEx:
    """one function of nqe_window_execute_ex's window: WindowFunction's functions and frames, ROWS BETWEEN `start` AND `end` (signed
    offsets from the current row, None: unbounded on that side) with frame WindowFrameEx.RowsBetween, lag / lead over `expr` by `offset`
    rows with an optional `default` (a ScalarValue of the argument's dtype — Q6: no coercion), first_value / last_value over `expr`
    and a frame, ntile over `buckets`"""

    def __init__(self, func: WindowFuncEx, expr: Optional[PhysicalExpr] = None, frame: WindowFrameEx = WindowFrameEx.Range, start: Optional[int] = None, end: Optional[int] = None,
                 offset: int = 1, buckets: int = 1, default: Optional[ScalarValue] = None):
        self.func, self.expr, self.frame = WindowFuncEx(func), expr, WindowFrameEx(frame)
        self.start, self.end, self.offset, self.buckets, self.default = start, end, int(offset), int(buckets), default
        if self.func not in _WINDOW_EX_NO_ARG and expr is None:
            raise ErrorCode(Status.PlanError, f"window function {_WINDOW_EX_LABELS[self.func]} needs an argument")

    @staticmethod
    def create(func: WindowFuncEx, expr: Optional[PhysicalExpr] = None, frame: WindowFrameEx = WindowFrameEx.Range, start: Optional[int] = None, end: Optional[int] = None,
               offset: int = 1, buckets: int = 1, default: Optional[ScalarValue] = None) -> "WindowFunctionEx":
        return WindowFunctionEx(func, expr, frame, start, end, offset, buckets, default)

    def data_field(self, schema: NaiveSchema) -> Field:
        label = _WINDOW_EX_LABELS[self.func]
        if self.func == WindowFuncEx.Ntile:
            return Field(f"ntile({self.buckets})", DType.UINT64, False)
        if self.func in _WINDOW_EX_NO_ARG:
            return Field(f"{label}()", DType.UINT64, False)
        arg = schema[self.expr.resolve(schema)].name if isinstance(self.expr, ColumnExpr) else repr(self.expr)
        if self.func in _WINDOW_EX_VALUE:
            dtype = _static_dtype(self.expr, schema)
            if self.default is not None and (self.default.dtype != dtype or self.default.value is None):
                raise ErrorCode(Status.IntervalError, f"{label}: the default is {self.default.dtype.name}, the argument {dtype.name}")
            return Field(f"{label}({arg}, {self.offset})" if self.func in (WindowFuncEx.Lag, WindowFuncEx.Lead) else f"{label}({arg})", dtype, True)
        return Field(f"{label}({arg})", DType.UINT64 if self.func == WindowFuncEx.Count else DType.FLOAT64, False)

    def spec(self, column: Optional[int]) -> dict:
        """the function as Context.window_ex takes it"""
        d = None if self.default is None else (float(self.default.value) if self.default.dtype == DType.FLOAT64 else int(self.default.value))
        return {"func": self.func, "column": column, "frame": self.frame, "start": self.start, "end": self.end,
                "param": self.buckets if self.func == WindowFuncEx.Ntile else self.offset, "default": d}

    def __repr__(self):
        return f"WindowFunctionEx({self.func.name}, {self.expr!r}, {self.frame.name}, {self.start}, {self.end}, {self.offset}, {self.buckets}, {self.default})"


class PhysicalWindowPlanEx(_WindowPlan):
    """PhysicalWindowPlan over nqe_window_execute_ex (quirk Q23): the same window, the same shape, for WindowFunctionEx's functions; the
    value functions' columns are nullable and have the argument's dtype, and a default of another dtype is refused before anything runs."""

    _entry, _fields_first = "window_ex", True


# ----------------------------------------------------------------------------- DISTINCT and the set operators
class PhysicalDistinctPlan(PhysicalPlan):
    """SELECT DISTINCT (quirk Q24; the reference's planner has no DISTINCT): the rows that are the first occurrence of their tuple
    over the expressions `on` (None: every column), in input order, with every input column.  Like PhysicalSortPlan the input batches
    are concatenated and ONE batch leaves.  A key that is a bare ColumnExpr is passed by index; any other expression is evaluated into
    a temporary column that never reaches the output."""

    def __init__(self, input: PhysicalPlan, on: Optional[Sequence[PhysicalExpr]] = None):
        self.input, self.on = input, None if on is None else list(on)

    @staticmethod
    def create(input: PhysicalPlan, on: Optional[Sequence[PhysicalExpr]] = None) -> "PhysicalDistinctPlan":
        return PhysicalDistinctPlan(input, on)

    def schema(self):
        return self.input.schema()

    def children(self):
        return [self.input]

    def execute(self):
        batches = self.input.execute()
        if not batches:
            raise ErrorCode(Status.NotSupported, "distinct over an empty batch list is not supported on the device path")
        ctx = _ctx_of(batches)
        fields = batches[0].fields
        kt = _KeyedTable(ctx, batches, fields)
        if self.on is None:
            return [DeviceRecordBatch(fields, ctx.distinct(kt.table))]
        cols = [kt.column_of(expr) for expr in self.on]
        return [DeviceRecordBatch(fields, kt.without_temps(ctx.distinct(kt.source(), cols)))]


class PhysicalSetOpPlan(PhysicalPlan):
    """UNION / INTERSECT / EXCEPT (quirk Q24; the reference's planner has no set operator): every column is a key, both inputs need the
    same column types.  The batches of each side are concatenated and ONE batch leaves, with left's schema."""

    def __init__(self, left: PhysicalPlan, right: PhysicalPlan, op: SetOp):
        self.left, self.right, self.op = left, right, SetOp(op)

    @staticmethod
    def create(left: PhysicalPlan, right: PhysicalPlan, op: SetOp) -> "PhysicalSetOpPlan":
        return PhysicalSetOpPlan(left, right, op)

    def schema(self):
        return self.left.schema()

    def children(self):
        return [self.left, self.right]

    def execute(self):
        lb, rb = self.left.execute(), self.right.execute()
        if not lb or not rb:
            raise ErrorCode(Status.NotSupported, "a set operation over an empty batch list is not supported on the device path")
        ctx = _ctx_of(lb)
        return [DeviceRecordBatch(lb[0].fields, ctx.set_op(_one_table(ctx, lb), _one_table(ctx, rb), self.op))]
