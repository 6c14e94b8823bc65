// test_order_by.cpp — ORDER BY (quirk Q18) through the C++ host mirror (naive_query_engine_amd/host/naive_db.hpp): the golden query
// `select * from employee order by department_id desc, rank` directly, with a LIMIT folded into the sort by the rewrite pass, with an
// expression key, and the operator's errors.  Expected rows: tests/golden/order_by_expected.json holds the same five.
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

struct Row { int64_t id; const char *name; int64_t department_id, rank; };
// department_id descending, then rank ascending
static const Row kGolden[5] = {{5, "mike", 3, 2}, {3, "Alex", 2, 0}, {4, "jack", 2, 1}, {2, "lynne", 1, 0}, {1, "vee", 1, 1}};

static void check_rows(const std::vector<RecordBatch> &out, int64_t rows) {
    CHECK(out.size() == 1);
    const RecordBatch &b = out[0];
    CHECK(b.num_rows() == rows && b.num_columns() == 4);
    const char *names[] = {"id", "name", "department_id", "rank"};
    for (size_t i = 0; i < 4; ++i) CHECK(b.schema().field(i).name() == names[i]);
    Array id = b.column(0), name = b.column(1), dep = b.column(2), rank = b.column(3);
    for (int64_t j = 0; j < rows; ++j) {
        const Row &r = kGolden[j];
        CHECK(id.i64(j) == r.id && name.str(j) == r.name && dep.i64(j) == r.department_id && rank.i64(j) == r.rank);
    }
}

int main(int argc, char **argv) {
    std::string dir = argc > 1 ? argv[1] : "tests/golden";
    TableRef employee = CsvTable::try_create(dir + "/employee.csv", CsvConfig());
    auto keys = [] {
        return std::vector<PhysicalSortExpr>{PhysicalSortExpr(ColumnExpr::try_create("department_id", std::nullopt), true, true),
                                             PhysicalSortExpr(ColumnExpr::try_create("rank", std::nullopt))};
    };

    run("order by department_id desc, rank: one batch, the input's schema", [&] {
        auto plan = PhysicalSortPlan::create(ScanPlan::create(employee, std::nullopt), keys());
        CHECK(plan->children().size() == 1 && plan->schema().fields().size() == 4);
        check_rows(plan->execute(), 5);
    });
    run("a LIMIT over the sort becomes its fetch in the rewrite pass; both forms give the same rows", [&] {
        auto tree = PhysicalLimitPlan::create(PhysicalSortPlan::create(ScanPlan::create(employee, std::nullopt), keys()), 3);
        check_rows(tree->execute(), 3);
        auto fused = std::dynamic_pointer_cast<PhysicalSortPlan>(rewrite(tree));
        CHECK(fused != nullptr && fused->fetch && *fused->fetch == 3);
        check_rows(fused->execute(), 3);
        NaiveDB db;
        check_rows(db.run_plan(tree), 3);
        auto off = rewrite(PhysicalOffsetPlan::create(PhysicalSortPlan::create(ScanPlan::create(employee, std::nullopt), keys()), 1));
        CHECK(std::dynamic_pointer_cast<PhysicalOffsetPlan>(off) != nullptr); // an offset over a sort stays as it is
    });
    run("an expression key is evaluated into a temporary column that the output drops", [&] {
        // 0 - department_id ascending = department_id descending
        auto neg = PhysicalBinaryExpr::create(PhysicalLiteralExpr::create(ScalarValue::Int64(0)), Operator::Minus, ColumnExpr::try_create("department_id", std::nullopt));
        std::vector<PhysicalSortExpr> k{PhysicalSortExpr(neg), PhysicalSortExpr(ColumnExpr::try_create("rank", std::nullopt))};
        check_rows(PhysicalSortPlan::create(ScanPlan::create(employee, std::nullopt), k)->execute(), 5);
    });
    run("no keys is a PlanError, a key index out of range NotSupported", [&] {
        try {
            PhysicalSortPlan::create(ScanPlan::create(employee, std::nullopt), {})->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::PlanError); }
        try {
            PhysicalSortPlan::create(ScanPlan::create(employee, std::nullopt), {PhysicalSortExpr(ColumnExpr::try_create(std::nullopt, size_t(9)))})->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::NotSupported); }
    });
    std::printf("%d/%d tests passed\n", g_run - g_failed, g_run);
    return g_failed ? 1 : 0;
}
