// test_nested_loop_join.cpp — the reference README's two-join query (README.md:77-85) with both joins as NestedLoopJoin through the
// C++ host mirror (naive_query_engine_amd/host/naive_db.hpp), directly and after the rewrite pass, plus quirk Q17's NULL keys and the
// operator's errors.  Expected rows: tests/golden/nested_loop_join_expected.json holds the same five, in outer-major order.
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

struct Row { int64_t id; const char *name, *rank_name, *department_name; };
static const Row kReadme[5] = {{1, "vee", "diamond", "IT"}, {2, "lynne", "master", "IT"}, {3, "Alex", "master", "Marketing"},
                               {4, "jack", "diamond", "Marketing"}, {5, "mike", "grandmaster", "Human Resource"}};

static void check_readme(const std::vector<RecordBatch> &out) {
    CHECK(out.size() == 1);
    const RecordBatch &b = out[0];
    CHECK(b.num_rows() == 5 && b.num_columns() == 8);
    const char *names[] = {"id", "name", "department_id", "rank", "id", "rank_name", "id", "department_name"};
    for (size_t i = 0; i < 8; ++i) CHECK(b.schema().field(i).name() == names[i]);
    Array id = b.column(0), name = b.column(1), rank_name = b.column(5), dep_name = b.column(7);
    for (int64_t j = 0; j < 5; ++j) {
        const Row &r = kReadme[j];
        CHECK(id.i64(j) == r.id && name.str(j) == r.name && rank_name.str(j) == r.rank_name && dep_name.str(j) == r.department_name);
    }
}

int main(int argc, char **argv) {
    std::string dir = argc > 1 ? argv[1] : "tests/golden";
    TableRef employee = CsvTable::try_create(dir + "/employee.csv", CsvConfig());
    TableRef rank = CsvTable::try_create(dir + "/rank.csv", CsvConfig());
    TableRef department = CsvTable::try_create(dir + "/department.csv", CsvConfig());
    std::vector<NaiveField> f1 = employee->schema().fields();
    for (auto &f : rank->schema().fields()) f1.push_back(f);
    std::vector<NaiveField> f2 = f1;
    for (auto &f : department->schema().fields()) f2.push_back(f);
    auto tree = [&] {
        auto j1 = NestedLoopJoin::create(ScanPlan::create(employee, std::nullopt), ScanPlan::create(rank, std::nullopt),
                                         {{Column{"employee", "rank"}, Column{"rank", "id"}}}, JoinType::Inner, NaiveSchema(f1));
        return NestedLoopJoin::create(j1, ScanPlan::create(department, std::nullopt), {{Column{"employee", "department_id"}, Column{"department", "id"}}},
                                      JoinType::Inner, NaiveSchema(f2));
    };

    run("README query 2 with both joins as NestedLoopJoin (outer-major order)", [&] { check_readme(tree()->execute()); });
    run("the same after the rewrite pass (NaiveDB::run_plan); a second execute() is identical", [&] {
        auto plan = rewrite(tree());
        auto top = std::dynamic_pointer_cast<NestedLoopJoin>(plan);
        CHECK(top != nullptr && std::dynamic_pointer_cast<NestedLoopJoin>(top->left) != nullptr);
        NaiveDB db;
        check_readme(db.run_plan(plan));
        check_readme(plan->execute());
    });
    run("NULL keys match nothing (quirk Q17)", [&] {
        NaiveSchema s({NaiveField(std::nullopt, "k", DataType::Int64, true)});
        Array l = Array::from_opt_i64({1, std::nullopt, 2, 1}), r = Array::from_opt_i64({std::nullopt, 1, 2});
        TableRef lt = MemTable::try_create(s, {RecordBatch::try_new(Context::default_context(), s, {l})});
        TableRef rt = MemTable::try_create(s, {RecordBatch::try_new(Context::default_context(), s, {r})});
        auto out = NestedLoopJoin::create(ScanPlan::create(lt, std::nullopt), ScanPlan::create(rt, std::nullopt), {{Column{"l", "k"}, Column{"r", "k"}}},
                                          JoinType::Inner, NaiveSchema(std::vector<NaiveField>{}))->execute();
        CHECK(out.size() == 1 && out[0].num_rows() == 3 && out[0].num_columns() == 2);
        CHECK(out[0].column(0).to_i64() == (std::vector<int64_t>{1, 2, 1}));
        CHECK(out[0].column(1).to_i64() == (std::vector<int64_t>{1, 2, 1}));
    });
    run("an empty `on` is a PlanError, key types that differ too", [&] {
        try {
            NestedLoopJoin::create(ScanPlan::create(employee, std::nullopt), ScanPlan::create(rank, std::nullopt), {}, JoinType::Inner, NaiveSchema(f1))->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::PlanError); }
        try {
            NestedLoopJoin::create(ScanPlan::create(employee, std::nullopt), ScanPlan::create(rank, std::nullopt), {{Column{"employee", "name"}, Column{"rank", "id"}}},
                                   JoinType::Inner, NaiveSchema(f1))->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::PlanError); }
    });
    std::printf("%d/%d tests passed\n", g_run - g_failed, g_run);
    return g_failed ? 1 : 0;
}
