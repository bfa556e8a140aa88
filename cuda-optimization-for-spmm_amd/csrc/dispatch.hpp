// Run-time value -> template argument, written once (host only).  A launcher names the values a template argument may
// take in ONE list; nothing else decides which instances exist.
//
//   with_acc<AccRefF32, AccFast>(acc_mode, [&](auto acc) {
//       using Acc = typename decltype(acc)::type;
//       with_vec(vec, [&](auto v) {
//           with_group(g, [&](auto gr) { launch_coo<decltype(gr)::value, decltype(v)::value, Acc>(a); });
//       });
//   });
//
// A value that comes from a knob_int() stays behind a plain `if` where the production library must not hold the other
// forms: the compiler folds such an `if` where it stands, and a kernel named only in the dead branch gets no host stub.
//
// Every helper is forced inline, so an entry point's dispatch compiles to the compare-and-branch chain it replaces.
#pragma once
#include <type_traits>

#include "mispmm.h"

namespace mispmm {

template <class T>
struct type_tag {
    using type = T;
};

// f(std::integral_constant<int, Vi>{}) for the Vi equal to v, for the LAST of the list where none is: what a switch's
// default: and a trailing else did.  Returns what f returns.
template <int V0, int... Vs, class F>
[[gnu::always_inline]] inline auto with_const(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
    else if (v == V0) return f(std::integral_constant<int, V0>{});
    else return with_const<Vs...>(v, f);
}

// the same, but a value outside the list calls nothing: false
template <int V0, int... Vs, class F>
[[gnu::always_inline]] inline bool try_const(int v, F &&f) {
    if (v == V0) return f(std::integral_constant<int, V0>{}), true;
    if constexpr (sizeof...(Vs) == 0) return false;
    else return try_const<Vs...>(v, f);
}

// lanes per row group
template <class F>
[[gnu::always_inline]] inline auto with_group(int g, F &&f) {
    return with_const<8, 16, 32, 64>(g, f);
}

// elements per lane of a 16-, 8- or 4-byte fp32 access
template <class F>
[[gnu::always_inline]] inline auto with_vec(int vec, F &&f) {
    return with_const<4, 2, 1>(vec, f);
}

template <class F>
[[gnu::always_inline]] inline auto with_flag(bool b, F &&f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// acc_mode has been validated (check_acc_mode): REFERENCE or FAST
template <class Ref, class Fast, class F>
[[gnu::always_inline]] inline auto with_acc(int acc_mode, F &&f) {
    return acc_mode == MISPMM_ACC_REFERENCE ? f(type_tag<Ref>{}) : f(type_tag<Fast>{});
}

}  // namespace mispmm
