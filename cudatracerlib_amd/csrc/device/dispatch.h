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

// The shading levels (template FULL of the shading kernels, DevScene::full_shading; shading.h says
// what each is for) and, one row per level, what a level carries: the traversal's alpha test, the
// environment light, the seven-type BSDF dispatch, the point / spot / distant lights, the medium, the
// sensor switch; and the level whose instantiation the kernels that never trace run for it (they have no alpha
// test to leave out, so alpha shares full's).  A new level is one row here and one entry in the
// level list of each site that instantiates it.
enum : int { kShadeLean = 0, kShadeFull = 1, kShadeEnv = 2, kShadeAlpha = 3, kShadeMat = 4, kShadeLights = 5, kShadeMedia = 6,
              kShadeSensors = 7 };
struct ShadeLevel { bool alpha, env, ext, delta_lights, media, sensors; int no_trace; };
constexpr ShadeLevel kShadeLevels[] = {
    /* lean   */ {false, false, false, false, false, false, kShadeLean},
    /* full   */ {false, false, false, false, false, false, kShadeFull},
    /* env    */ {true, true, false, false, false, false, kShadeEnv},
    /* alpha  */ {true, false, false, false, false, false, kShadeFull},
    /* mat    */ {true, true, true, false, false, false, kShadeMat},
    /* lights */ {true, true, true, true, false, false, kShadeLights},
    /* media  */ {true, true, true, true, true, false, kShadeMedia},
    /* sensors*/ {true, true, true, true, true, true, kShadeSensors},
};
// kShadeLevelCount: the levels that differ in what they shade (lean ... media).  kShadeSensors shades what
// media shades and differs in where the primary ray comes from; it is the table's last row, past that count.
constexpr int kShadeLevelCount = kShadeMedia + 1;
constexpr int kLevelRows = sizeof(kShadeLevels) / sizeof(kShadeLevels[0]);
static_assert(kLevelRows == kShadeSensors + 1, "one row per level");
// a value that is no level carries nothing and maps to itself
constexpr bool shade_level_known(int l) { return l >= 0 && l < kLevelRows; }
constexpr bool level_alpha(int l) { return shade_level_known(l) && kShadeLevels[l].alpha; }
constexpr bool level_env(int l) { return shade_level_known(l) && kShadeLevels[l].env; }
constexpr bool level_ext(int l) { return shade_level_known(l) && kShadeLevels[l].ext; }
constexpr bool level_delta_lights(int l) { return shade_level_known(l) && kShadeLevels[l].delta_lights; }
constexpr bool level_media(int l) { return shade_level_known(l) && kShadeLevels[l].media; }
constexpr bool level_sensors(int l) { return shade_level_known(l) && kShadeLevels[l].sensors; }
constexpr int level_no_trace(int l) { return shade_level_known(l) ? kShadeLevels[l].no_trace : l; }

// The level a scene runs, by precedence sensors > media > lights > mat > env > alpha > full > lean: each scene
// runs the lowest level that carries all it holds, so a scene without a feature keeps the kernels it
// had before the feature existed.  shaded: some material is not a plain constant diffuse one
// (another BSDF type, a texture, an alpha state); alpha: some material has an alpha state; env: an
// environment light; ext: some material is of the five ext BSDF types; delta_light: a point, spot or
// distant light; volume: a participating medium; sensor: a sensor other than the perspective one (thin
// lens, orthographic, telecentric, spherical).  material_level is the part the materials and the
// environment decide, which ctl_ctx keeps between uploads that change neither.
constexpr int material_level(bool shaded, bool alpha, bool env, bool ext) {
    return ext ? kShadeMat : env ? kShadeEnv : alpha ? kShadeAlpha : shaded ? kShadeFull : kShadeLean;
}
constexpr int scene_level(int materials, bool delta_light, bool volume, bool sensor = false) {
    return sensor ? kShadeSensors : volume ? kShadeMedia : delta_light ? kShadeLights : materials;
}
constexpr int scene_level(bool shaded, bool alpha, bool env, bool ext, bool delta_light, bool volume, bool sensor = false) {
    return scene_level(material_level(shaded, alpha, env, ext), delta_light, volume, sensor);
}

}  // namespace ctl
