// dispatch.h — run-time scene properties -> the compile-time switches of the
// traced kernels.  Each entry point calls a generic lambda with constants
// (std::bool_constant / std::integral_constant) that the launch site uses as
// decltype(X)::value in the kernel's template-id.  Plain C++17, no HIP or
// project header: tests/test_dispatch.py builds it with the host compiler.
#pragma once
#include <type_traits>

namespace ctl {

// f(SG, WD): SINGLE = one-level scene, WIDE = 1 the 4-wide tree, 0 the binary one.
template <class F>
void with_tree(bool single, bool wide, F&& f) {
    using B = std::integral_constant<int, 0>;
    using W = std::integral_constant<int, 1>;
    if (wide) { if (single) f(std::true_type{}, W{}); else f(std::false_type{}, W{}); }
    else { if (single) f(std::true_type{}, B{}); else f(std::false_type{}, B{}); }
}

// f(ST, SG, WD) for the kernels with a STATS variant.  Stats launches count the
// reference's binary traversal (the roofline's algorithmic bytes), whatever
// tree the scene renders with: STATS with WIDE = 1 is never instantiated.
template <class F>
void with_tree(bool stats, bool single, bool wide, F&& f) {
    using B = std::integral_constant<int, 0>;
    if (!stats) return with_tree(single, wide, [&](auto SG, auto WD) { f(std::false_type{}, SG, WD); });
    if (single) f(std::true_type{}, std::true_type{}, B{}); else f(std::true_type{}, std::false_type{}, B{});
}

// f(FU) for the listed shading level equal to `full`; false (and no call) when
// none is: the list is the set of levels the site instantiates.
template <int... L, class F>
bool with_level(int full, F&& f) {
    return ((full == L && (f(std::integral_constant<int, L>{}), true)) || ...);
}

}  // namespace ctl
