// nb_dispatch.h -- runtime value -> template argument, for the host launchers.  Host only; builds with a plain C++17 compiler.
//
//   return nb::pick<2, 3>(dim, [&](auto D) {
//       return nb::pick<1, 2, 4>(r, [&](auto R) {
//           hipLaunchKernelGGL((kernel<D.value, R.value>), ...);
//           return hipGetLastError();
//       });
//   });
//
// A value outside the candidate list runs nothing and yields hipErrorInvalidValue, so a launcher rejects bad input before
// it launches.  A sparse set of instantiations is a separate candidate list per branch, or an `if constexpr` inside the
// callable that returns hipErrorInvalidValue.
#pragma once
#include <hip/hip_runtime_api.h>

#include <type_traits>

namespace nb {

// f(std::integral_constant<..., Vk>{}) for the one candidate equal to `value`; returns what f returns
template <auto... Vs, typename T, typename F>
hipError_t pick(T value, F &&f)
{
    hipError_t err = hipErrorInvalidValue;
    (void)((value == Vs ? (err = f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
    return err;
}

// any non-zero flag is true (pick<true, false> would compare an int flag of 2 with `true`)
template <typename F>
hipError_t pick_bool(bool flag, F &&f)
{
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

template <typename T>
struct real_tag {
    using type = T;
};

// f(real_tag<double>{}) or f(real_tag<float>{}): `using T = typename decltype(real)::type;`
template <typename F>
hipError_t pick_real(bool is_f64, F &&f)
{
    return is_f64 ? f(real_tag<double>{}) : f(real_tag<float>{});
}

// The ladder under `dim` of the launchers that run the one-launch step's bodies (the nb_ens step kernels): f(S, BS, STOPS)
// for 64 / 32 / 16 lanes per target, a workgroup of one of BLOCKS threads, and a kernel with or without a stop array (or
// whatever else the launcher's last bool chooses).  dim stays the launcher's own outermost pick<2, 3>: the typed launchers
// choose the storage type and the hook between the two, and the kernels leave the compiler in the order of the nesting.
template <auto... BLOCKS, typename F>
hipError_t pick_small_step(int lanes, int block, bool stops, F &&f)
{
    return pick<64, 32, 16>(lanes, [&](auto S) {
        return pick<BLOCKS...>(block, [&](auto BS) {
            return pick_bool(stops, [&](auto ST) { return f(S, BS, ST); });
        });
    });
}

}  // namespace nb
