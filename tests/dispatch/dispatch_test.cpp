// Host-only test of csrc/nb_dispatch.h: nb::pick / nb::pick_bool / nb::pick_real hand the callable the right compile-time
// constant exactly once, run nothing for a value outside the list, and pass the callable's error code through.
// Built and run by tests/test_dispatch_header.py with the host compiler; needs no GPU.
#include "nb_dispatch.h"

#include <cstdio>
#include <type_traits>

static int failures = 0;
#define CHECK(...)                                                               \
    do {                                                                         \
        if (!(__VA_ARGS__)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__);   \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

enum Hook { HOOK_A = 0, HOOK_B = 1, HOOK_C = 3 };

template <int D, int R>
struct Pair {
    static constexpr int code = D * 10 + R;
};

int main()
{
    // every candidate: the callable runs exactly once, with that constant
    for (int v : {16, 32, 64}) {
        int calls = 0, seen = -1;
        const hipError_t e = nb::pick<64, 32, 16>(v, [&](auto S) {
            static_assert(std::is_same_v<typename decltype(S)::value_type, int>);
            ++calls;
            seen = S.value;
            return hipSuccess;
        });
        CHECK(e == hipSuccess && calls == 1 && seen == v);
    }
    // a value that is not listed: nothing runs, hipErrorInvalidValue
    for (int v : {0, 8, 48, -16, 65}) {
        int calls = 0;
        const hipError_t e = nb::pick<64, 32, 16>(v, [&](auto) { ++calls; return hipSuccess; });
        CHECK(e == hipErrorInvalidValue && calls == 0);
    }
    // a single candidate, negative candidates, enumerators (also mixed with plain integers)
    {
        int calls = 0;
        CHECK(nb::pick<7>(7, [&](auto V) { calls += V.value; return hipSuccess; }) == hipSuccess && calls == 7);
        CHECK(nb::pick<7>(6, [&](auto) { ++calls; return hipSuccess; }) == hipErrorInvalidValue && calls == 7);
        int seen = 99;
        CHECK(nb::pick<-1, HOOK_B, HOOK_C>(-1, [&](auto V) { seen = (int)V.value; return hipSuccess; }) == hipSuccess && seen == -1);
        CHECK(nb::pick<-1, HOOK_B, HOOK_C>((int)HOOK_C, [&](auto V) { seen = (int)V.value; return hipSuccess; }) == hipSuccess &&
              seen == 3);
        CHECK(nb::pick<-1, HOOK_B, HOOK_C>((int)HOOK_A, [&](auto V) { seen = (int)V.value; return hipSuccess; }) ==
                  hipErrorInvalidValue && seen == 3);
    }
    // the callable's own error code comes back unchanged, and only the matching candidate produced it
    {
        int calls = 0;
        const hipError_t e = nb::pick<2, 3>(3, [&](auto D) {
            ++calls;
            return D.value == 3 ? hipErrorOutOfMemory : hipErrorUnknown;
        });
        CHECK(e == hipErrorOutOfMemory && calls == 1);
        CHECK(nb::pick_bool(true, [](auto) { return hipErrorNotReady; }) == hipErrorNotReady);
        CHECK(nb::pick_real(false, [](auto) { return hipErrorNotReady; }) == hipErrorNotReady);
    }
    // nested picks reach the right pair, once; a bad inner or outer value reaches none
    for (int d : {1, 2, 3, 4})
        for (int r : {0, 1, 2, 3, 4}) {
            int calls = 0, code = -1;
            const hipError_t e = nb::pick<2, 3>(d, [&](auto D) {
                return nb::pick<1, 2, 4>(r, [&](auto R) {
                    ++calls;
                    code = Pair<D.value, R.value>::code;       // the constants are usable as template arguments
                    return hipSuccess;
                });
            });
            const bool ok = (d == 2 || d == 3) && (r == 1 || r == 2 || r == 4);
            CHECK(e == (ok ? hipSuccess : hipErrorInvalidValue));
            CHECK(calls == (ok ? 1 : 0) && code == (ok ? d * 10 + r : -1));
        }
    // a sparse product: `if constexpr` leaves out a pair without instantiating it
    {
        int calls = 0;
        auto sparse = [&](int d, int r) {
            return nb::pick<2, 3>(d, [&](auto D) {
                return nb::pick<2, 4>(r, [&](auto R) {
                    if constexpr (D.value == 3 && R.value == 4) return hipErrorInvalidValue;
                    else { ++calls; return hipSuccess; }
                });
            });
        };
        CHECK(sparse(3, 4) == hipErrorInvalidValue && calls == 0);
        CHECK(sparse(3, 2) == hipSuccess && sparse(2, 4) == hipSuccess && calls == 2);
    }
    // pick_bool: any non-zero flag is true
    for (int flag : {0, 1, 2, -1}) {
        int calls = 0;
        bool seen = false;
        CHECK(nb::pick_bool(flag, [&](auto B) { ++calls; seen = B.value; return hipSuccess; }) == hipSuccess);
        CHECK(calls == 1 && seen == (flag != 0));
    }
    // pick_real: double for true, float for false
    for (int is_f64 : {0, 1, 5}) {
        int calls = 0;
        size_t bytes = 0;
        bool is_double = false, is_float = false;
        const hipError_t e = nb::pick_real(is_f64, [&](auto real) {
            using T = typename decltype(real)::type;
            ++calls;
            bytes = sizeof(T);
            is_double = std::is_same_v<T, double>;
            is_float = std::is_same_v<T, float>;
            return hipSuccess;
        });
        CHECK(e == hipSuccess && calls == 1);
        CHECK(is_f64 ? (is_double && !is_float && bytes == 8) : (is_float && !is_double && bytes == 4));
    }
    if (failures) return 1;
    std::printf("nb_dispatch.h: all checks passed\n");
    return 0;
}
