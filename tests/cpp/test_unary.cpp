// test_unary.cpp — the reference's two unary unit tests (test_abs_expression / test_sin_expression, unary.rs:122-170: abs(score)
// and sin(score) over data/test_data.csv) through the C++ host mirror's PhysicalUnaryExpr (naive_query_engine_amd/host/naive_db.hpp),
// quirk Q16 (Tan evaluates the cosine) and the unimplemented!() child types.  Expected values: tests/golden/unary_expected.json.
#include <cmath>
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

// distance between two doubles in units in the last place (ordered bit patterns)
static int64_t ulps(double a, double b) {
    auto ord = [](double d) { int64_t i; std::memcpy(&i, &d, 8); return i < 0 ? INT64_MIN - i : i; };
    int64_t x = ord(a), y = ord(b);
    return x > y ? x - y : y - x;
}

static const double kAbs[8] = {60.0, 90.1, 99.99, 81.1, 82.2, 83.3, 84.4, 85.5};
static const double kSin[8] = {-0.3048106211022167, 0.8447976840197418, -0.5149633680424761, -0.5492019627147913,
                               0.49565689358989423, 0.9988580516952367, 0.4104993826174394, -0.6264561960895026};

int main(int argc, char **argv) {
    std::string dir = argc > 1 ? argv[1] : "tests/golden";
    TableRef table = CsvTable::try_create(dir + "/test_data.csv", CsvConfig());
    NaiveSchema out_schema({NaiveField(std::nullopt, "x", DataType::Float64, false)});
    auto project = [&](PhysicalExprRef e) {
        auto out = ProjectionPlan::create(ScanPlan::create(table, std::nullopt), out_schema, {std::move(e)})->execute();
        CHECK(out.size() == 1 && out[0].num_rows() == 8 && out[0].num_columns() == 1);
        Array a = out[0].column(0);
        CHECK(a.dtype == DataType::Float64);
        return a;
    };
    auto score = [] { return ColumnExpr::try_create(std::string("score"), std::nullopt); };

    run("test_abs_expression (unary.rs:122-145): bit-exact", [&] {
        Array a = project(PhysicalUnaryExpr::create(score(), UnaryOperator::Abs, "abs", DataType::Float64));
        for (int64_t j = 0; j < 8; ++j) CHECK(a.is_valid(j) && ulps(a.f64(j), kAbs[j]) == 0);
    });
    run("test_sin_expression (unary.rs:147-170): within 5 ulp of the recorded vector (4 ulp device library + 1 ulp host library)", [&] {
        // name / return_type as the planner passes them (planner/mod.rs:208-217): stored, ignored
        Array a = project(PhysicalUnaryExpr::create(score(), UnaryOperator::Sin, "todo", DataType::Int64));
        for (int64_t j = 0; j < 8; ++j) CHECK(a.is_valid(j) && ulps(a.f64(j), kSin[j]) <= 5);
    });
    run("quirk Q16: Tan evaluates the cosine (unary.rs:96), bit for bit what Cos gives", [&] {
        Array t = project(PhysicalUnaryExpr::create(score(), UnaryOperator::Tan, "tan", DataType::Float64));
        Array c = project(PhysicalUnaryExpr::create(score(), UnaryOperator::Cos, "cos", DataType::Float64));
        for (int64_t j = 0; j < 8; ++j) CHECK(ulps(t.f64(j), c.f64(j)) == 0 && ulps(t.f64(j), std::cos(kAbs[j])) <= 5);
    });
    run("an Int64 child and a string function are NotSupported (unimplemented!() / todo!())", [&] {
        for (auto e : {PhysicalUnaryExpr::create(ColumnExpr::try_create(std::string("age"), std::nullopt), UnaryOperator::Abs, "abs", DataType::Int64),
                       PhysicalUnaryExpr::create(score(), UnaryOperator::Lower, "lower", DataType::Utf8)}) {
            try {
                ProjectionPlan::create(ScanPlan::create(table, std::nullopt), out_schema, {e})->execute();
                CHECK(false);
            } catch (const ErrorCode &err) { CHECK(err.status == ErrorCode::NotSupported); }
        }
    });
    std::printf("%d/%d tests passed\n", g_run - g_failed, g_run);
    return g_failed ? 1 : 0;
}
