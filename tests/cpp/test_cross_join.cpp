// test_cross_join.cpp — the reference README's third query (`select * from employee join rank`, README.md:86-104) through the
// C++ host mirror's CrossJoin (naive_query_engine_amd/host/naive_db.hpp), directly and after the rewrite pass.  Expected rows: the
// 15 the README prints (tests/golden/readme_cross_join.json holds the same rows).
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

struct Row { int64_t id; const char *name; int64_t department_id, rank, id2; const char *rank_name; };
static const Row kReadme[15] = {
    {1, "vee", 1, 1, 1, "master"},        {2, "lynne", 1, 0, 2, "diamond"},     {3, "Alex", 2, 0, 3, "grandmaster"},
    {4, "jack", 2, 1, 4, "master"},       {5, "mike", 3, 2, 5, "diamond"},      {1, "vee", 1, 1, 1, "grandmaster"},
    {2, "lynne", 1, 0, 2, "master"},      {3, "Alex", 2, 0, 3, "diamond"},      {4, "jack", 2, 1, 4, "grandmaster"},
    {5, "mike", 3, 2, 5, "master"},       {1, "vee", 1, 1, 1, "diamond"},       {2, "lynne", 1, 0, 2, "grandmaster"},
    {3, "Alex", 2, 0, 3, "master"},       {4, "jack", 2, 1, 4, "diamond"},      {5, "mike", 3, 2, 5, "grandmaster"},
};

static void check_readme(const std::vector<RecordBatch> &out) {
    CHECK(out.size() == 1);
    const RecordBatch &b = out[0];
    CHECK(b.num_rows() == 15 && b.num_columns() == 6);
    const char *names[] = {"id", "name", "department_id", "rank", "id", "rank_name"};
    for (size_t i = 0; i < 6; ++i) CHECK(b.schema().field(i).name() == names[i]);
    Array id = b.column(0), name = b.column(1), dep = b.column(2), rank = b.column(3), id2 = b.column(4), rank_name = b.column(5);
    for (int64_t j = 0; j < 15; ++j) {
        const Row &r = kReadme[j];
        CHECK(id.i64(j) == r.id && name.str(j) == r.name && dep.i64(j) == r.department_id && rank.i64(j) == r.rank);
        CHECK(id2.i64(j) == r.id2 && rank_name.str(j) == r.rank_name);
    }
}

int main(int argc, char **argv) {
    std::string dir = argc > 1 ? argv[1] : "tests/golden";
    TableRef employee = CsvTable::try_create(dir + "/employee.csv", CsvConfig());
    TableRef rank = CsvTable::try_create(dir + "/rank.csv", CsvConfig());
    std::vector<NaiveField> fields = employee->schema().fields();
    for (auto &f : rank->schema().fields()) fields.push_back(f);
    NaiveSchema join_schema(fields);
    auto tree = [&] {
        auto join = CrossJoin::create(ScanPlan::create(employee, std::nullopt), ScanPlan::create(rank, std::nullopt), JoinType::Cross, join_schema);
        std::vector<PhysicalExprRef> star; // `select *`: every field by name, the first match (the second `id` is employee.id)
        for (auto &f : fields) star.push_back(ColumnExpr::try_create(f.name(), std::nullopt));
        return ProjectionPlan::create(join, join_schema, star);
    };

    run("README query 3: select * from employee join rank (cross_join.rs, quirk Q15)", [&] { check_readme(tree()->execute()); });
    run("the same after the rewrite pass (NaiveDB::run_plan)", [&] {
        auto plan = rewrite(tree());
        CHECK(std::dynamic_pointer_cast<CrossJoin>(std::dynamic_pointer_cast<ProjectionPlan>(plan)->input) != nullptr);
        NaiveDB db;
        check_readme(db.run_plan(plan));
    });
    run("a Boolean column is NotSupported (cross_join.rs: unimplemented!())", [&] {
        Array flag;
        flag.dtype = DataType::Boolean;
        flag.length = 2;
        flag.bits = {0x1};
        NaiveSchema s({NaiveField(std::nullopt, "flag", DataType::Boolean, false)});
        TableRef t = MemTable::try_create(s, {RecordBatch::try_new(Context::default_context(), s, {flag})});
        try {
            CrossJoin::create(ScanPlan::create(employee, std::nullopt), ScanPlan::create(t, std::nullopt), JoinType::Cross, join_schema)->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::NotSupported); }
    });
    std::printf("%d/%d tests passed\n", g_run - g_failed, g_run);
    return g_failed ? 1 : 0;
}
