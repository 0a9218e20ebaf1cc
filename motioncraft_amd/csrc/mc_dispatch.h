// Host side: one way from a runtime L / mode / split value to the kernel instantiation for it (the launchers of mc_chain.hip
// and mc_half.hip).  A launcher lists exactly the values it instantiates:
//     const bool ok = mc_dispatch<128, 64, 32>(g.L, [&](auto L) {
//         mc_dispatch<0, 1>(split, [&](auto S) { hipLaunchKernelGGL((kernel_k<MC_V(L), bool(MC_V(S))>), grid, block, 0, s, args); });
//     });
#pragma once
#include <type_traits>

// f(std::integral_constant<int, V>{}) for the V among VS that equals v; false (nothing called) when none does
template <int... VS, class F>
inline bool mc_dispatch(int v, F&& f) {
    return ((v == VS && (f(std::integral_constant<int, VS>{}), true)) || ...);
}
// the compile-time value of a dispatched argument (usable where the argument itself, a lambda parameter, is not a constant expression)
#define MC_V(x) (std::remove_reference_t<decltype(x)>::value)
