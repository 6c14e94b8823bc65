// nqe_error.hpp — the library's one exception type.  Plain C++17, no HIP: the headers that compile on their own (expr_plan.hpp) raise
// errors through it; nqe_internal.hpp includes it, so every unit sees it as before.
#pragma once

#include <string>

namespace nqe {

struct Error {
    int code;
    std::string msg;
};

[[noreturn]] inline void fail(int code, const std::string &msg) { throw Error{code, msg}; }

} // namespace nqe
