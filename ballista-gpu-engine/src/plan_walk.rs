//! DataFusion physical plan -> the JSON mirror of `PhysicalPlanNode` that `gpuq_plan_create` executes
//! (grammar: include/gpuq.h "native plan executor"; node / field names follow ballista/core/proto/datafusion.proto).
//!
//! Nodes are recognised the way the reference does it itself: `as_any().downcast_ref::<T>()`
//! (ballista/core/src/physical_optimizer/task_group.rs:143-167, ballista/core/src/utils.rs:274-311).  A subtree the
//! device path does not execute (an unbounded window, an expression outside the supported subset, a scan the native leaves do not
//! cover) is NOT an error: it becomes a *host leaf* -- the shim runs that subtree with DataFusion as the stock executor
//! would and hands its batches to the device through the Arrow C Data Interface (`gpuq_table_import_arrow`), as input
//! slot k of a `MemoryExec` node.
//!
//! Scans: `ParquetExec` / `CsvExec` over the local file system map to the native leaves of the same names (file groups
//! with their byte ranges, projection, limit, the pruning predicate through the expression walker): the file bytes cross
//! PCIe once and are decoded on the device.  A scan over another object store, with table_partition_cols, an
//! output_ordering or a CSV escape character stays a host leaf.  (This mapping was written without a Rust toolchain at
//! hand, like the rest of this crate: it has not been compiled.)
use std::sync::Arc;

use ballista_core::execution_plans::{CoalesceTasksExec, ShuffleReaderExec, ShuffleWriterExec};
use datafusion::arrow::datatypes::{DataType, SchemaRef};
use datafusion::common::{DataFusionError, Result, ScalarValue};
use datafusion::datasource::physical_plan::{CsvExec, FileScanConfig, ParquetExec};
use datafusion::execution::object_store::ObjectStoreUrl;
use datafusion::logical_expr::Operator;
use datafusion::physical_expr::ScalarFunctionExpr;
use datafusion::physical_plan::aggregates::{AggregateExec, AggregateMode};
use datafusion::physical_plan::coalesce_batches::CoalesceBatchesExec;
use datafusion::physical_plan::coalesce_partitions::CoalescePartitionsExec;
use datafusion::physical_plan::expressions::{
    ApproxDistinct, Avg, BinaryExpr, BitAnd, BitOr, BitXor, BoolAnd, BoolOr, CaseExpr, CastExpr, Column, Count, DistinctBitXor, DistinctCount, DistinctSum, InListExpr, IsNotNullExpr, IsNullExpr, LikeExpr, Literal, Max, Median, Min, NegativeExpr, NotExpr,
    PhysicalSortExpr, Sum, TryCastExpr,
};
use datafusion::physical_plan::filter::FilterExec;
use datafusion::physical_plan::joins::{CrossJoinExec, HashJoinExec, PartitionMode};
use datafusion::physical_plan::limit::{GlobalLimitExec, LocalLimitExec};
use datafusion::physical_plan::projection::ProjectionExec;
use datafusion::physical_plan::sorts::sort::SortExec;
use datafusion::physical_plan::sorts::sort_preserving_merge::SortPreservingMergeExec;
use datafusion::physical_plan::union::UnionExec;
use datafusion::logical_expr::{WindowFrameBound, WindowFrameUnits};
use datafusion::physical_plan::windows::{BoundedWindowAggExec, BuiltInWindowExpr, PartitionSearchMode, PlainAggregateWindowExpr, SlidingAggregateWindowExpr};
use datafusion::physical_expr::window::{Rank, RankType, RowNumber, WindowExpr, WindowShift};
use datafusion::physical_plan::{AggregateExpr, ExecutionPlan, Partitioning, PhysicalExpr};
use serde_json::{json, Value};

/// What `walk` produces: the plan JSON plus the subtrees the host must run and feed in as input slots.
pub struct WalkedPlan {
    pub json: Value,
    /// host_leaves[k] = (subtree, partition of it) feeds input slot k
    pub host_leaves: Vec<(Arc<dyn ExecutionPlan>, usize)>,
}

pub fn walk_stage(writer: &ShuffleWriterExec, job_id: &str, stage_id: usize, work_dir: &str) -> Result<WalkedPlan> {
    let mut leaves = vec![];
    let input = walk(&writer.children()[0], &mut leaves)?;
    let mut node = json!({"input": input, "job_id": job_id, "stage_id": stage_id, "work_dir": work_dir,
                          "partitions": writer.partitions()});
    if let Some(Partitioning::Hash(exprs, n)) = writer.shuffle_output_partitioning() {
        let he: Result<Vec<Value>> = exprs.iter().map(expr).collect();
        node["output_partitioning"] = json!({"hash_expr": he?, "partition_count": n});
    }
    Ok(WalkedPlan { json: json!({"ShuffleWriterExec": node}), host_leaves: leaves })
}

fn unsupported<T>(what: impl Into<String>) -> Result<T> {
    Err(DataFusionError::NotImplemented(what.into()))
}

pub fn type_json(t: &DataType) -> Result<Value> {
    Ok(match t {
        DataType::Boolean => json!("Boolean"),
        DataType::Int32 => json!("Int32"),
        DataType::Int64 => json!("Int64"),
        DataType::UInt32 => json!("UInt32"),
        DataType::UInt64 => json!("UInt64"),
        DataType::Date32 => json!("Date32"),
        DataType::Float64 => json!("Float64"),
        DataType::Utf8 => json!("Utf8"),
        DataType::Decimal128(p, s) => json!({"Decimal128": [p, s]}),
        DataType::Int8 => json!("Int8"),
        DataType::Int16 => json!("Int16"),
        DataType::UInt8 => json!("UInt8"),
        DataType::UInt16 => json!("UInt16"),
        DataType::Float32 => json!("Float32"),
        DataType::Date64 => json!("Date64"),
        // the engine keeps the unit; the zone travels in the descriptor and comes back with this plan's schema (batches are built with it)
        DataType::Timestamp(u, tz) => json!({"Timestamp": [format!("{u:?}"), tz.as_ref().map(|z| z.to_string())]}),
        // a span of its unit: carried like a Timestamp (an Interval is a literal only: no arm here, a field of that type is refused)
        DataType::Duration(u) => json!({"Duration": format!("{u:?}")}),
        // converted where the batches enter (gpuq_table_import_arrow / gpuq_ingest_push): inside, 32-bit offsets / the value type
        DataType::LargeUtf8 => json!("LargeUtf8"),
        DataType::Dictionary(k, v) => json!({"Dictionary": [type_json(k)?, type_json(v)?]}),
        other => return unsupported(format!("column type {other:?}")),
    })
}

pub fn schema_json(s: &SchemaRef) -> Result<Value> {
    let f: Result<Vec<Value>> = s.fields().iter().map(|f| Ok(json!({"name": f.name(), "type": type_json(f.data_type())?, "nullable": f.is_nullable()}))).collect();
    Ok(Value::Array(f?))
}

fn literal(v: &ScalarValue) -> Result<Value> {
    // decimals travel as the unscaled integer in a string; NULL literals keep their type
    Ok(match v {
        ScalarValue::Boolean(x) => json!({"type": "Boolean", "value": x}),
        ScalarValue::Int32(x) => json!({"type": "Int32", "value": x}),
        ScalarValue::Int64(x) => json!({"type": "Int64", "value": x}),
        ScalarValue::UInt32(x) => json!({"type": "UInt32", "value": x}),
        ScalarValue::UInt64(x) => json!({"type": "UInt64", "value": x}),
        ScalarValue::Date32(x) => json!({"type": "Date32", "value": x}),
        ScalarValue::Float64(x) => json!({"type": "Float64", "value": x}),
        ScalarValue::Utf8(x) => json!({"type": "Utf8", "value": x}),
        ScalarValue::LargeUtf8(x) => json!({"type": "Utf8", "value": x}),
        ScalarValue::Int8(x) => json!({"type": "Int8", "value": x}),
        ScalarValue::Int16(x) => json!({"type": "Int16", "value": x}),
        ScalarValue::UInt8(x) => json!({"type": "UInt8", "value": x}),
        ScalarValue::UInt16(x) => json!({"type": "UInt16", "value": x}),
        ScalarValue::Float32(x) => json!({"type": "Float32", "value": x}),
        ScalarValue::Date64(x) => json!({"type": "Date64", "value": x.map(|v| v.to_string())}),
        ScalarValue::TimestampSecond(x, tz) => json!({"type": {"Timestamp": ["Second", tz.as_ref().map(|z| z.to_string())]}, "value": x.map(|v| v.to_string())}),
        ScalarValue::TimestampMillisecond(x, tz) => json!({"type": {"Timestamp": ["Millisecond", tz.as_ref().map(|z| z.to_string())]}, "value": x.map(|v| v.to_string())}),
        ScalarValue::TimestampMicrosecond(x, tz) => json!({"type": {"Timestamp": ["Microsecond", tz.as_ref().map(|z| z.to_string())]}, "value": x.map(|v| v.to_string())}),
        ScalarValue::TimestampNanosecond(x, tz) => json!({"type": {"Timestamp": ["Nanosecond", tz.as_ref().map(|z| z.to_string())]}, "value": x.map(|v| v.to_string())}),
        // the three IntervalUnits in their parts (arrow packs DayTime as days << 32 | milliseconds and MonthDayNano as
        // months << 96 | days << 64 | nanoseconds: to_parts undoes that), the four Durations as their count
        ScalarValue::IntervalYearMonth(x) => json!({"type": {"Interval": "YearMonth"}, "value": x.map(|v| v.to_string())}),
        ScalarValue::IntervalDayTime(x) => json!({"type": {"Interval": "DayTime"}, "value": x.map(|v| {
            let (days, milliseconds) = arrow::datatypes::IntervalDayTimeType::to_parts(v);
            json!({"days": days, "milliseconds": milliseconds})
        })}),
        ScalarValue::IntervalMonthDayNano(x) => json!({"type": {"Interval": "MonthDayNano"}, "value": x.map(|v| {
            let (months, days, nanoseconds) = arrow::datatypes::IntervalMonthDayNanoType::to_parts(v);
            json!({"months": months, "days": days, "nanoseconds": nanoseconds.to_string()})
        })}),
        ScalarValue::DurationSecond(x) => json!({"type": {"Duration": "Second"}, "value": x.map(|v| v.to_string())}),
        ScalarValue::DurationMillisecond(x) => json!({"type": {"Duration": "Millisecond"}, "value": x.map(|v| v.to_string())}),
        ScalarValue::DurationMicrosecond(x) => json!({"type": {"Duration": "Microsecond"}, "value": x.map(|v| v.to_string())}),
        ScalarValue::DurationNanosecond(x) => json!({"type": {"Duration": "Nanosecond"}, "value": x.map(|v| v.to_string())}),
        ScalarValue::Decimal128(x, p, s) => json!({"type": {"Decimal128": [p, s]}, "value": x.map(|v| v.to_string())}),
        other => return unsupported(format!("literal {other:?}")),
    })
}

fn binary_op(op: &Operator) -> Result<&'static str> {
    // PhysicalBinaryExprNode.op travels as the operator's name (datafusion.proto:1228-1232)
    Ok(match op {
        Operator::Plus => "Plus", Operator::Minus => "Minus", Operator::Multiply => "Multiply", Operator::Divide => "Divide", Operator::Modulo => "Modulo",
        Operator::Eq => "Eq", Operator::NotEq => "NotEq", Operator::Lt => "Lt", Operator::LtEq => "LtEq", Operator::Gt => "Gt", Operator::GtEq => "GtEq",
        Operator::And => "And", Operator::Or => "Or",
        // two integers of one type (the planner has inserted the casts); the shifts stay on the host
        Operator::BitwiseAnd => "BitwiseAnd", Operator::BitwiseOr => "BitwiseOr", Operator::BitwiseXor => "BitwiseXor",
        other => return unsupported(format!("binary operator {other:?}")),
    })
}

/// PhysicalExprNode mirror (datafusion.proto:1142-1180).
pub fn expr(e: &Arc<dyn PhysicalExpr>) -> Result<Value> {
    let a = e.as_any();
    if let Some(c) = a.downcast_ref::<Column>() {
        return Ok(json!({"column": {"name": c.name(), "index": c.index()}}));
    }
    if let Some(l) = a.downcast_ref::<Literal>() {
        return Ok(json!({"literal": literal(l.value())?}));
    }
    if let Some(b) = a.downcast_ref::<BinaryExpr>() {
        return Ok(json!({"binary_expr": {"l": expr(b.left())?, "r": expr(b.right())?, "op": binary_op(b.op())?}}));
    }
    if let Some(c) = a.downcast_ref::<CastExpr>() {
        return Ok(json!({"cast": {"expr": expr(c.expr())?, "arrow_type": type_json(c.cast_type())?}}));
    }
    if let Some(c) = a.downcast_ref::<TryCastExpr>() {
        return Ok(json!({"try_cast": {"expr": expr(c.expr())?, "arrow_type": type_json(c.cast_type())?}}));
    }
    if let Some(x) = a.downcast_ref::<IsNullExpr>() {
        return Ok(json!({"is_null_expr": {"expr": expr(x.arg())?}}));
    }
    if let Some(x) = a.downcast_ref::<IsNotNullExpr>() {
        return Ok(json!({"is_not_null_expr": {"expr": expr(x.arg())?}}));
    }
    if let Some(x) = a.downcast_ref::<NotExpr>() {
        return Ok(json!({"not_expr": {"expr": expr(x.arg())?}}));
    }
    if let Some(x) = a.downcast_ref::<NegativeExpr>() {
        return Ok(json!({"negative": {"expr": expr(x.arg())?}}));
    }
    if let Some(x) = a.downcast_ref::<InListExpr>() {
        let list: Result<Vec<Value>> = x.list().iter().map(expr).collect();
        return Ok(json!({"in_list": {"expr": expr(x.expr())?, "list": list?, "negated": x.negated()}}));
    }
    if let Some(x) = a.downcast_ref::<CaseExpr>() {
        let wt: Result<Vec<Value>> = x.when_then_expr().iter().map(|(w, t)| Ok(json!({"when_expr": expr(w)?, "then_expr": expr(t)?}))).collect();
        let base = match x.expr() { Some(b) => expr(b)?, None => Value::Null };
        let els = match x.else_expr() { Some(b) => expr(b)?, None => Value::Null };
        return Ok(json!({"case_": {"expr": base, "when_then_expr": wt?, "else_expr": els}}));
    }
    if let Some(x) = a.downcast_ref::<LikeExpr>() {
        return Ok(json!({"like_expr": {"negated": x.negated(), "case_insensitive": x.case_insensitive(), "expr": expr(x.expr())?, "pattern": expr(x.pattern())?}}));
    }
    if let Some(x) = a.downcast_ref::<ScalarFunctionExpr>() {
        // PhysicalScalarFunctionNode: the names the device's expression compiler builds (csrc/expr_compile.cpp, which checks the argument
        // types and refuses by message); every other function keeps its subtree on the host
        const BUILT: [&str; 16] = ["date_part", "datepart", "substr", "substring", "coalesce", "nullif", "nanvl", "isnan", "iszero", "abs", "signum", "ceil", "floor",
                                   "trunc", "round", "sqrt"];
        let name = x.name().to_ascii_lowercase();
        if !BUILT.contains(&name.as_str()) {
            return unsupported(format!("scalar function {name}"));
        }
        let args: Result<Vec<Value>> = x.args().iter().map(expr).collect();
        return Ok(json!({"scalar_function": {"name": name, "args": args?}}));
    }
    unsupported(format!("physical expression {e:?}"))
}

fn sort_exprs(v: &[PhysicalSortExpr]) -> Result<Value> {
    let r: Result<Vec<Value>> = v.iter().map(|s| Ok(json!({"expr": expr(&s.expr)?, "asc": !s.options.descending, "nulls_first": s.options.nulls_first}))).collect();
    Ok(Value::Array(r?))
}

/// One bound of a window frame (WindowFrameBound, datafusion.proto:791-799): a NULL scalar is UNBOUNDED.
fn frame_bound(b: &WindowFrameBound) -> Result<Value> {
    let rows = |v: &ScalarValue| -> Result<Value> {
        if v.is_null() { return Ok(Value::Null); }
        match v {
            ScalarValue::UInt64(Some(x)) => Ok(json!(x)),
            ScalarValue::Int64(Some(x)) => Ok(json!(x)),
            other => unsupported(format!("window frame offset {other:?}")),      // a RANGE offset in the order key's type
        }
    };
    Ok(match b {
        WindowFrameBound::Preceding(v) => json!({"type": "PRECEDING", "value": rows(v)?}),
        WindowFrameBound::CurrentRow => json!({"type": "CURRENT_ROW", "value": Value::Null}),
        WindowFrameBound::Following(v) => json!({"type": "FOLLOWING", "value": rows(v)?}),
    })
}

/// PhysicalWindowExprNode mirror (datafusion.proto:1198-1209) for the functions the native BoundedWindowAggExec runs; anything else keeps
/// the node on the host.  [UPSTREAM-KNOWLEDGE: datafusion 34 physical-expr window/{built_in, rank, row_number, lead_lag, aggregate,
/// sliding_aggregate}.rs -- LAG holds a positive shift offset, LEAD a negative one.]
fn window_expr(w: &Arc<dyn WindowExpr>) -> Result<Value> {
    let x = w.as_any();
    // (is_agg: only the aggregate functions read their frame; the ranks' and LAG / LEAD's is left out, whatever scalars its bounds hold)
    let mut is_agg = false;
    let (name, args): (&str, Vec<Value>) = if let Some(b) = x.downcast_ref::<BuiltInWindowExpr>() {
        let f = b.get_built_in_func_expr();
        let fa = f.as_any();
        if fa.is::<RowNumber>() { ("ROW_NUMBER", vec![]) }
        else if let Some(r) = fa.downcast_ref::<Rank>() {
            match r.get_type() { RankType::Basic => ("RANK", vec![]), RankType::Dense => ("DENSE_RANK", vec![]), RankType::Percent => return unsupported("PERCENT_RANK") }
        } else if let Some(s) = fa.downcast_ref::<WindowShift>() {
            let off = s.get_shift_offset();
            let mut a = vec![expr(&f.expressions()[0])?, json!({"literal": {"type": "Int64", "value": off.abs()}})];
            if let Some(d) = s.get_default_value() { a.push(json!({"literal": literal(&d)?})); }
            (if off >= 0 { "LAG" } else { "LEAD" }, a)
        } else { return unsupported(format!("window function {}", f.name())) }
    } else {
        let agg = if let Some(p) = x.downcast_ref::<PlainAggregateWindowExpr>() { p.get_aggregate_expr() }
                  else if let Some(p) = x.downcast_ref::<SlidingAggregateWindowExpr>() { p.get_aggregate_expr() }
                  else { return unsupported(format!("window expression {}", w.name())) };
        let name = aggregate_fn(agg)?;
        if !["COUNT", "SUM", "MIN", "MAX", "AVG"].contains(&name) { return unsupported(format!("window aggregate {name}")); }
        let a: Result<Vec<Value>> = agg.expressions().iter().map(expr).collect();
        is_agg = true;
        (name, a?)
    };
    let pb: Result<Vec<Value>> = w.partition_by().iter().map(expr).collect();
    let fr = w.get_window_frame();
    let units = match fr.units { WindowFrameUnits::Rows => "ROWS", WindowFrameUnits::Range => "RANGE", WindowFrameUnits::Groups => "GROUPS" };
    let mut j = json!({"fn": name, "args": args, "partition_by": pb?, "order_by": sort_exprs(w.order_by())?, "name": w.name()});
    if is_agg {
        j["window_frame"] = json!({"units": units, "start_bound": frame_bound(&fr.start_bound)?, "end_bound": frame_bound(&fr.end_bound)?});
    }
    Ok(j)
}

fn aggregate_fn(a: &Arc<dyn AggregateExpr>) -> Result<&'static str> {
    let x = a.as_any();
    Ok(if x.is::<Sum>() { "SUM" } else if x.is::<Avg>() { "AVG" } else if x.is::<Count>() { "COUNT" } else if x.is::<Min>() { "MIN" } else if x.is::<Max>() { "MAX" }
       else if x.is::<BitAnd>() { "BIT_AND" } else if x.is::<BitOr>() { "BIT_OR" } else if x.is::<BitXor>() { "BIT_XOR" }
       else if x.is::<BoolAnd>() { "BOOL_AND" } else if x.is::<BoolOr>() { "BOOL_OR" }
       else if x.is::<Median>() { "MEDIAN" }      // mode Single only: the native executor lowers it in the plan (include/gpuq.h) and refuses the other modes
       else if x.is::<ApproxDistinct>() { "APPROX_DISTINCT" }      // mode Single only, as MEDIAN: lowered in the plan (a HyperLogLog sketch per segment); its two-phase state is refused
       else { return unsupported(format!("aggregate {}", a.name())) })
}

/// agg(DISTINCT x) as DataFusion 34 plans it beside other aggregates: an accumulator of its own that keeps the group's set of values.  The
/// JSON carries the plain function's name plus `"distinct": true`; the native executor lowers the node (mode Single only; include/gpuq.h,
/// gpuq_segment_distinct, has the rules) and refuses the other modes by name.
fn distinct_aggregate_fn(a: &Arc<dyn AggregateExpr>) -> Option<&'static str> {
    let x = a.as_any();
    if x.is::<DistinctCount>() { Some("COUNT") } else if x.is::<DistinctSum>() { Some("SUM") } else if x.is::<DistinctBitXor>() { Some("BIT_XOR") } else { None }
}

/// One plan node.  On `NotImplemented` from anything below, the caller turns the WHOLE subtree rooted here into a host leaf.
fn walk_node(p: &Arc<dyn ExecutionPlan>, leaves: &mut Vec<(Arc<dyn ExecutionPlan>, usize)>) -> Result<Value> {
    let a = p.as_any();
    if let Some(n) = a.downcast_ref::<CoalesceBatchesExec>() {
        return Ok(json!({"CoalesceBatchesExec": {"input": walk(n.input(), leaves)?}}));
    }
    if let Some(n) = a.downcast_ref::<FilterExec>() {
        return Ok(json!({"FilterExec": {"input": walk(n.input(), leaves)?, "expr": expr(n.predicate())?}}));
    }
    if let Some(n) = a.downcast_ref::<ProjectionExec>() {
        let e: Result<Vec<Value>> = n.expr().iter().map(|(e, _)| expr(e)).collect();
        let names: Vec<&str> = n.expr().iter().map(|(_, s)| s.as_str()).collect();
        return Ok(json!({"ProjectionExec": {"input": walk(n.input(), leaves)?, "expr": e?, "expr_name": names}}));
    }
    if let Some(n) = a.downcast_ref::<AggregateExec>() {
        let mode = match n.mode() {
            AggregateMode::Partial => "Partial", AggregateMode::Final => "Final", AggregateMode::FinalPartitioned => "FinalPartitioned",
            AggregateMode::Single => "Single", AggregateMode::SinglePartitioned => "Single",
        };
        let final_ = matches!(n.mode(), AggregateMode::Final | AggregateMode::FinalPartitioned);
        let ge: Result<Vec<Value>> = n.group_expr().expr().iter().map(|(e, name)| Ok(json!({"expr": expr(e)?, "name": name}))).collect();
        let mut ae = vec![];
        for agg in n.aggr_expr() {
            let mut o = match distinct_aggregate_fn(agg) {
                Some(f) => json!({"fn": f, "name": agg.name(), "distinct": true}),
                None => json!({"fn": aggregate_fn(agg)?, "name": agg.name()}),
            };
            if !final_ {
                // Final modes read the state columns of the Partial stage by position: no argument expressions
                let args = agg.expressions();
                if let Some(e0) = args.first() { o["expr"] = expr(e0)?; }
                if let Some(e1) = args.get(1) { o["expr2"] = expr(e1)?; }
            }
            ae.push(o);
        }
        if n.filter_expr().iter().any(|f| f.is_some()) { return unsupported("aggregate FILTER clause"); }
        let mut node = json!({"input": walk(n.input(), leaves)?, "mode": mode, "group_expr": ge?, "aggr_expr": ae});
        // Grouping sets (ROLLUP / CUBE / GROUPING SETS): `groups` is one Vec<bool> per set, true = the key is NULL in that set, and null_expr
        // the typed NULLs.  The one all-false set of a plain GROUP BY is left out; an ungrouped node has no group expressions and no sets.
        // The executor lowers the node (include/gpuq.h, gpuq_grouping_expand) and refuses what it does not run, loudly.
        let groups = n.group_expr().groups();
        if !n.group_expr().expr().is_empty() && !(groups.len() == 1 && groups[0].iter().all(|masked| !*masked)) {
            let ne: Result<Vec<Value>> = n.group_expr().null_expr().iter().map(|(e, _)| expr(e)).collect();
            node["groups"] = json!(groups);
            node["null_expr"] = json!(ne?);
        }
        return Ok(json!({"AggregateExec": node}));
    }
    if let Some(n) = a.downcast_ref::<HashJoinExec>() {
        let on: Vec<Value> = n.on().iter().map(|(l, r)| json!({"left": {"column": {"name": l.name(), "index": l.index()}},
                                                                "right": {"column": {"name": r.name(), "index": r.index()}}})).collect();
        let mode = match n.partition_mode() { PartitionMode::CollectLeft => "CollectLeft", PartitionMode::Partitioned => "Partitioned", PartitionMode::Auto => "CollectLeft" };
        let mut j = json!({"left": walk(n.left(), leaves)?, "right": walk(n.right(), leaves)?, "on": on, "join_type": format!("{:?}", n.join_type()),
                           "partition_mode": mode, "null_equals_null": n.null_equals_null()});
        if let Some(f) = n.filter() {
            // JoinFilter.expression is written against the intermediate schema (column_indices); the device evaluates it over
            // the joined row, so columns are re-pointed at (side, index) -> position in left ++ right
            j["filter"] = crate::plan_walk::join_filter(f, n.left().schema().fields().len())?;
        }
        return Ok(json!({"HashJoinExec": j}));
    }
    if let Some(n) = a.downcast_ref::<CrossJoinExec>() {
        // (an uncorrelated scalar subquery arrives as a one-row left side; gpuq refuses more than 2^32 pairs)
        return Ok(json!({"CrossJoinExec": {"left": walk(n.left(), leaves)?, "right": walk(n.right(), leaves)?}}));
    }
    if let Some(n) = a.downcast_ref::<BoundedWindowAggExec>() {
        // The bounded-frame window node, in mode Sorted only: the input is ordered by (partition_by, order_by), which is all the native node
        // asks for.  Linear / PartiallySorted, the unbounded WindowAggExec and the functions window_expr does not name stay host leaves; a
        // frame or an argument type the device refuses (include/gpuq.h lists them) is refused loudly by gpuq_plan_create, as any refusal is.
        if !matches!(n.partition_search_mode, PartitionSearchMode::Sorted) {
            return unsupported("BoundedWindowAggExec in a partition_search_mode other than Sorted");
        }
        let we: Result<Vec<Value>> = n.window_expr().iter().map(window_expr).collect();
        return Ok(json!({"BoundedWindowAggExec": {"input": walk(n.input(), leaves)?, "window_expr": we?, "partition_search_mode": "Sorted"}}));
    }
    if let Some(n) = a.downcast_ref::<SortExec>() {
        if n.preserve_partitioning() && n.input().output_partitioning().partition_count() > 1 {
            // per-partition sort: one task covers the partitions CoalesceTasksExec hands it; the native SortExec sorts what it is given
        }
        return Ok(json!({"SortExec": {"input": walk(n.input(), leaves)?, "expr": sort_exprs(n.expr())?, "fetch": n.fetch().map(|f| f as i64).unwrap_or(-1)}}));
    }
    if let Some(n) = a.downcast_ref::<SortPreservingMergeExec>() {
        return Ok(json!({"SortPreservingMergeExec": {"input": walk(n.input(), leaves)?, "expr": sort_exprs(n.expr())?, "fetch": n.fetch().map(|f| f as i64).unwrap_or(-1)}}));
    }
    if let Some(n) = a.downcast_ref::<CoalescePartitionsExec>() {
        return Ok(json!({"CoalescePartitionsExec": {"input": walk(n.input(), leaves)?}}));
    }
    if let Some(n) = a.downcast_ref::<UnionExec>() {
        let ins: Result<Vec<Value>> = n.inputs().iter().map(|i| walk(i, leaves)).collect();
        return Ok(json!({"UnionExec": {"inputs": ins?}}));
    }
    if let Some(n) = a.downcast_ref::<LocalLimitExec>() {
        return Ok(json!({"LocalLimitExec": {"input": walk(n.input(), leaves)?, "fetch": n.fetch()}}));
    }
    if let Some(n) = a.downcast_ref::<GlobalLimitExec>() {
        return Ok(json!({"GlobalLimitExec": {"input": walk(n.input(), leaves)?, "skip": n.skip(), "fetch": n.fetch().map(|f| f as i64).unwrap_or(-1)}}));
    }
    if let Some(n) = a.downcast_ref::<CoalesceTasksExec>() {
        let mut j = json!({"input": walk(&n.children()[0], leaves)?, "partitions": n.partitions()});
        if let Some(ob) = n.order_by() { j["order_by"] = sort_exprs(ob)?; }
        return Ok(json!({"CoalesceTasksExec": j}));
    }
    if let Some(n) = a.downcast_ref::<ShuffleReaderExec>() {
        // local files are decoded on the device; a location that is not on this node's filesystem ("local" is decided exactly
        // as the reference does, Path::exists, shuffle_reader.rs:626-628) makes the reader a host leaf: DataFusion's
        // ShuffleReaderExec fetches it over Flight and the batches are imported
        let mut parts = vec![];
        for locs in &n.partition {
            let mut files = vec![];
            for l in locs {
                if l.partition_stats.num_rows() == Some(0) { continue; }                 // shuffle_reader.rs:251
                if !std::path::Path::new(&l.path).exists() { return unsupported("remote shuffle location"); }
                files.push(json!({"path": l.path}));
            }
            parts.push(Value::Array(files));
        }
        return Ok(json!({"ShuffleReaderExec": {"schema": schema_json(&n.schema())?, "partition": parts}}));
    }
    if let Some(n) = a.downcast_ref::<ParquetExec>() {
        let mut j = file_scan(n.base_config())?;
        // the pruning predicate is over the FILE schema, by name; the FilterExec above the leaf applies it to rows.  A predicate the
        // expression walker does not carry is dropped, not the scan: pruning is an optimisation, the filter is what decides
        if let Some(pred) = n.predicate() {
            if let Ok(e) = expr(pred) { j["predicate"] = e; }
        }
        return Ok(json!({"ParquetExec": j}));
    }
    if let Some(n) = a.downcast_ref::<CsvExec>() {
        if n.escape().is_some() { return unsupported("CsvExec with an escape character"); }
        let mut j = file_scan(n.base_config())?;
        j["has_header"] = json!(n.has_header());
        j["delimiter"] = json!(one_byte(n.delimiter())?);
        j["quote"] = json!(one_byte(n.quote())?);
        return Ok(json!({"CsvExec": j}));
    }
    unsupported(format!("plan node {}", p.name()))
}

fn one_byte(b: u8) -> Result<String> {
    // the grammar carries the byte as a one-byte JSON string: ASCII only
    if b.is_ascii() { Ok((b as char).to_string()) } else { unsupported("a CSV delimiter / quote outside ASCII") }
}

/// FileScanExecConf (datafusion.proto) of a scan over local files -> the members ParquetExec / CsvExec share in the grammar.
/// Anything else -- another object store, partition columns, a declared output ordering -- keeps the scan a host leaf.
fn file_scan(c: &FileScanConfig) -> Result<Value> {
    if c.object_store_url != ObjectStoreUrl::local_filesystem() { return unsupported("a scan over an object store other than the local file system"); }
    if !c.table_partition_cols.is_empty() { return unsupported("a scan with table_partition_cols"); }
    if !c.output_ordering.is_empty() { return unsupported("a scan with an output_ordering"); }
    let mut groups = vec![];
    for g in &c.file_groups {
        let mut files = vec![];
        for f in g {
            if !f.partition_values.is_empty() { return unsupported("a partitioned file with partition values"); }
            // object_store paths of the local file system are absolute paths without their leading '/'
            let mut o = json!({"path": format!("/{}", f.object_meta.location.as_ref())});
            if let Some(r) = &f.range { o["range"] = json!([r.start, r.end]); }
            files.push(o);
        }
        groups.push(Value::Array(files));
    }
    let mut j = json!({"file_groups": groups, "schema": schema_json(&c.file_schema)?});
    if let Some(p) = &c.projection { j["projection"] = json!(p); }
    if let Some(l) = c.limit { j["limit"] = json!(l); }
    Ok(j)
}

pub fn walk(p: &Arc<dyn ExecutionPlan>, leaves: &mut Vec<(Arc<dyn ExecutionPlan>, usize)>) -> Result<Value> {
    let mark = leaves.len();
    match walk_node(p, leaves) {
        Ok(v) => Ok(v),
        Err(DataFusionError::NotImplemented(why)) => {
            // this subtree stays on the host: forget host leaves collected below it, it becomes one leaf itself
            leaves.truncate(mark);
            log::debug!("gpuq: subtree rooted at {} runs on the host ({why})", p.name());
            let nparts = p.output_partitioning().partition_count();
            let mut slots = vec![];
            for k in 0..nparts { slots.push(leaves.len()); leaves.push((p.clone(), k)); }      // input slot = position in host_leaves
            Ok(json!({"MemoryExec": {"schema": schema_json(&p.schema())?, "partitions": slots}}))
        }
        Err(e) => Err(e),
    }
}

/// JoinFilter -> expression over the joined row (left columns, then right columns).
pub fn join_filter(f: &datafusion::physical_plan::joins::utils::JoinFilter, n_left: usize) -> Result<Value> {
    use datafusion::common::JoinSide;
    let v = expr(f.expression())?;
    let idx = f.column_indices();
    fn remap(v: &mut Value, idx: &[datafusion::physical_plan::joins::utils::ColumnIndex], n_left: usize) {
        match v {
            Value::Object(m) => {
                if let Some(Value::Object(c)) = m.get_mut("column") {
                    if let Some(i) = c.get("index").and_then(|i| i.as_u64()) {
                        let ci = &idx[i as usize];
                        let pos = if ci.side == JoinSide::Left { ci.index } else { n_left + ci.index };
                        c.insert("index".into(), json!(pos));      // the native executor resolves by NAME: a filter over two sides that
                                                                     // share a column name is refused there (GPUQ_ERR_INVALID), not mis-bound
                    }
                    return;
                }
                for (_, x) in m.iter_mut() { remap(x, idx, n_left); }
            }
            Value::Array(a) => for x in a.iter_mut() { remap(x, idx, n_left); },
            _ => {}
        }
    }
    let mut v = v;
    remap(&mut v, idx, n_left);
    Ok(v)
}
