// test_outer_join.cpp — outer hash joins (quirk Q19) through the C++ host mirror (naive_query_engine_amd/host/naive_db.hpp): the golden
// queries over the rank / department / employee tables for Left, Right and Inner, a second execute() of one plan object, the rewrite
// arm, a probe side without batches and the operator's errors.  Expected rows: tests/golden/outer_join_expected.json holds the same.
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

// rank ⋈ department on id: {rank id, rank_name, department id, department_name}; a null name pointer = the NULL-extended side
struct Row { int64_t lid; const char *lname; int64_t rid; const char *rname; };

static void check_batch(const RecordBatch &b, const std::vector<Row> &rows) {
    CHECK(b.num_rows() == int64_t(rows.size()) && b.num_columns() == 4);
    const char *names[] = {"id", "rank_name", "id", "department_name"};
    for (size_t i = 0; i < 4; ++i) CHECK(b.schema().field(i).name() == names[i]);
    Array lid = b.column(0), lname = b.column(1), rid = b.column(2), rname = b.column(3);
    for (size_t j = 0; j < rows.size(); ++j) {
        const Row &r = rows[j];
        const int64_t i = int64_t(j);
        CHECK(lid.is_valid(i) == (r.lname != nullptr) && lname.is_valid(i) == (r.lname != nullptr));
        CHECK(rid.is_valid(i) == (r.rname != nullptr) && rname.is_valid(i) == (r.rname != nullptr));
        if (r.lname) CHECK(lid.i64(i) == r.lid && lname.str(i) == r.lname);
        else CHECK(lid.i64(i) == 0 && lname.str(i).empty()); // a NULL-extended cell holds 0 / the empty string
        if (r.rname) CHECK(rid.i64(i) == r.rid && rname.str(i) == r.rname);
        else CHECK(rid.i64(i) == 0 && rname.str(i).empty());
    }
}

int main(int argc, char **argv) {
    std::string dir = argc > 1 ? argv[1] : "tests/golden";
    TableRef rank = CsvTable::try_create(dir + "/rank.csv", CsvConfig());
    TableRef department = CsvTable::try_create(dir + "/department.csv", CsvConfig());
    auto on = [] { return std::vector<std::pair<Column, Column>>{{Column{std::nullopt, "id"}, Column{std::nullopt, "id"}}}; };
    auto join = [&](JoinType jt) { return HashOuterJoin::create(ScanPlan::create(rank, std::nullopt), ScanPlan::create(department, std::nullopt), on(), jt, NaiveSchema()); };
    const std::vector<Row> matched = {{1, "diamond", 1, "IT"}, {2, "grandmaster", 2, "Marketing"}};

    run("rank left join department: the inner rows, then the build rows that never matched", [&] {
        auto plan = join(JoinType::Left);
        CHECK(plan->children().size() == 2);
        for (int execution = 0; execution < 2; ++execution) { // nothing is kept between execute() calls
            auto out = plan->execute();
            CHECK(out.size() == 2);
            check_batch(out[0], matched);
            check_batch(out[1], {{0, "master", 0, nullptr}});
        }
    });
    run("rank right join department: an unmatched probe row emits one row with the left columns NULL", [&] {
        auto out = join(JoinType::Right)->execute();
        CHECK(out.size() == 1);
        check_batch(out[0], {{1, "diamond", 1, "IT"}, {2, "grandmaster", 2, "Marketing"}, {0, nullptr, 3, "Human Resource"}});
    });
    run("inner: the inner join's rows; the rewrite pass keeps the operator with rewritten children", [&] {
        auto out = join(JoinType::Inner)->execute();
        CHECK(out.size() == 1);
        check_batch(out[0], matched);
        auto re = std::dynamic_pointer_cast<HashOuterJoin>(rewrite(join(JoinType::Left)));
        CHECK(re != nullptr && re->join_type == JoinType::Left && re->children().size() == 2);
        NaiveDB db;
        auto viadb = db.run_plan(join(JoinType::Right));
        CHECK(viadb.size() == 1 && viadb[0].num_rows() == 3);
    });
    run("a probe side without rows: Left gives every build row with the right columns NULL", [&] {
        auto none = PhysicalLimitPlan::create(ScanPlan::create(department, std::nullopt), 0);
        auto out = HashOuterJoin::create(ScanPlan::create(rank, std::nullopt), none, on(), JoinType::Left, NaiveSchema())->execute();
        CHECK(!out.empty());
        check_batch(out.back(), {{0, "master", 0, nullptr}, {1, "diamond", 0, nullptr}, {2, "grandmaster", 0, nullptr}});
        for (size_t i = 0; i + 1 < out.size(); ++i) CHECK(out[i].num_rows() == 0);
    });
    run("Cross and an empty `on` are PlanErrors", [&] {
        try { join(JoinType::Cross)->execute(); CHECK(false); } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::PlanError); }
        try {
            HashOuterJoin::create(ScanPlan::create(rank, std::nullopt), ScanPlan::create(department, std::nullopt), {}, JoinType::Left, NaiveSchema())->execute();
            CHECK(false);
        } catch (const ErrorCode &e) { CHECK(e.status == ErrorCode::PlanError); }
    });
    std::printf("%d/%d tests passed\n", g_run - g_failed, g_run);
    return g_failed ? 1 : 0;
}
