// test_group_keys.cpp — GROUP BY on several keys (quirk Q20) through the C++ host mirror (naive_query_engine_amd/host/naive_db.hpp): the
// golden query `group by id % 3, age` over test_data.csv directly, under a selection (fused by the rewrite pass and unfused), with a Utf8
// key, and the operator's errors.  Expected rows: tests/golden/group_keys_expected.json holds the same ones.
#include <cstdio>
#include <functional>

#include "../../naive_query_engine_amd/host/naive_db.hpp"

using namespace naive_db;

static int g_failed = 0, g_run = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) { std::printf("  CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); throw 1; } \
    } while (0)

static void run(const char *name, const std::function<void()> &f) {
    ++g_run;
    try { f(); std::printf("ok   %s\n", name); }
    catch (const ErrorCode &e) { ++g_failed; std::printf("FAIL %s: ErrorCode %d %s\n", name, e.status, e.what()); }
    catch (...) { ++g_failed; std::printf("FAIL %s\n", name); }
}

// id % 3, age, count(score), sum(score), min(id), max(score): every tuple of the file is distinct, sorted by the tuple
struct Row { int64_t g0, age; uint64_t count; double sum, min_id, max; };
static const Row kGolden[8] = {{0, 20, 1, 82.2, 6.0, 82.2},  {0, 23, 1, 85.5, 9.0, 85.5}, {1, 18, 1, 99.99, 4.0, 99.99}, {1, 21, 1, 83.3, 7.0, 83.3},
                               {1, 23, 1, 60.0, 1.0, 60.0},  {2, 19, 1, 81.1, 5.0, 81.1}, {2, 20, 1, 90.1, 2.0, 90.1},   {2, 22, 1, 84.4, 8.0, 84.4}};

static void check_rows(const std::vector<RecordBatch> &out, int64_t min_age) {
    CHECK(out.size() == 1);
    const RecordBatch &b = out[0];
    CHECK(b.num_columns() == 6);
    const char *names[] = {"group_0", "age", "count(score)", "sum(score)", "min(id)", "max(score)"};
    for (size_t i = 0; i < 6; ++i) CHECK(b.schema().field(i).name() == names[i]);
    CHECK(b.schema().field(0).data_type == DataType::Int64 && b.schema().field(2).data_type == DataType::UInt64);
    Array g0 = b.column(0), age = b.column(1), cnt = b.column(2), sum = b.column(3), mn = b.column(4), mx = b.column(5);
    CHECK(g0.validity.empty() && age.validity.empty());
    int64_t j = 0;
    for (const Row &r : kGolden) {
        if (r.age <= min_age) continue;
        CHECK(j < b.num_rows());
        CHECK(g0.i64(j) == r.g0 && age.i64(j) == r.age && cnt.u64(j) == r.count && sum.f64(j) == r.sum && mn.f64(j) == r.min_id && mx.f64(j) == r.max);
        ++j;
    }
    CHECK(j == b.num_rows());
}

int main(int argc, char **argv) {
    std::string dir = argc > 1 ? argv[1] : "tests/golden";
    TableRef data = CsvTable::try_create(dir + "/test_data.csv", CsvConfig());
    auto col = [](const char *n) { return ColumnExpr::try_create(std::string(n), std::nullopt); };
    auto keys = [&] {
        return std::vector<PhysicalExprRef>{PhysicalBinaryExpr::create(col("id"), Operator::Modulos, PhysicalLiteralExpr::create(ScalarValue::Int64(3))), col("age")};
    };
    auto ops = [&] {
        std::vector<std::unique_ptr<AggregateOperator>> v;
        v.push_back(Count::create(col("score")));
        v.push_back(Sum::create(col("score")));
        v.push_back(Min::create(col("id")));
        v.push_back(Max::create(col("score")));
        return v;
    };

    run("group by id % 3, age: one batch, group fields then aggregate fields, sorted by the tuple", [&] {
        auto plan = GroupedAggregatePlan::create(keys(), ops(), ScanPlan::create(data, std::nullopt));
        CHECK(plan->children().size() == 1 && plan->schema().fields().size() == 6 && plan->schema().field(1).name() == "age");
        check_rows(plan->execute(), 0);
        check_rows(plan->execute(), 0); // nothing is kept between calls
    });
    run("under a selection: the rewrite pass fuses the predicate into the call; both forms give the same rows", [&] {
        auto pred = PhysicalBinaryExpr::create(col("age"), Operator::Gt, PhysicalLiteralExpr::create(ScalarValue::Int64(19)));
        auto tree = GroupedAggregatePlan::create(keys(), ops(), SelectionPlan::create(ScanPlan::create(data, std::nullopt), pred));
        check_rows(tree->execute(), 19);
        auto fused = std::dynamic_pointer_cast<FusedSelectionGroupedAggregatePlan>(rewrite(tree));
        CHECK(fused != nullptr && fused->predicate == pred && std::dynamic_pointer_cast<ScanPlan>(fused->input) != nullptr);
        check_rows(fused->execute(), 19);
        NaiveDB db;
        check_rows(db.run_plan(tree), 19);
        // the reference's own aggregate keeps its operator (Q8)
        auto old = rewrite(PhysicalAggregatePlan::create(keys(), ops(), SelectionPlan::create(ScanPlan::create(data, std::nullopt), pred)));
        CHECK(std::dynamic_pointer_cast<FusedSelectionAggregatePlan>(old) != nullptr && std::dynamic_pointer_cast<GroupedAggregatePlan>(old) == nullptr);
    });
    run("a Utf8 key beside an integer key", [&] {
        std::vector<PhysicalExprRef> k{col("name"), col("age")};
        auto out = GroupedAggregatePlan::create(k, ops(), ScanPlan::create(data, std::nullopt))->execute();
        CHECK(out.size() == 1 && out[0].num_rows() == 8 && out[0].schema().field(0).name() == "name" && out[0].schema().field(0).data_type == DataType::Utf8);
        Array name = out[0].column(0), age = out[0].column(1), sum = out[0].column(3);
        const char *sorted[] = {"alex", "alice", "bob", "cock", "jack", "lynne", "primer", "veeupup"};
        for (int64_t j = 0; j < 8; ++j) CHECK(name.str(j) == sorted[j]);
        CHECK(age.i64(0) == 20 && sum.f64(0) == 90.1 && age.i64(7) == 23 && sum.f64(7) == 60.0);
    });
    run("no keys is a PlanError, nine keys NotSupported, a Float64 key NotSupported", [&] {
        try {
            GroupedAggregatePlan::create({}, ops(), ScanPlan::create(data, std::nullopt));
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::PlanError); }
        try {
            std::vector<PhysicalExprRef> nine(9, col("age"));
            GroupedAggregatePlan::create(nine, ops(), ScanPlan::create(data, std::nullopt))->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::NotSupported); }
        try {
            std::vector<PhysicalExprRef> k{col("age"), col("score")};
            GroupedAggregatePlan::create(k, ops(), ScanPlan::create(data, std::nullopt))->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::NotSupported); }
    });
    std::printf("%d/%d tests passed\n", g_run - g_failed, g_run);
    return g_failed ? 1 : 0;
}
