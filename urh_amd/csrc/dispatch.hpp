// Run-time value -> template argument, stated once for every launch site (host code only).
//
//     return dispatch_dtype(dtype, [&](auto dt) {
//         return dispatch_mod<URHGPU_MOD_ASK, URHGPU_MOD_FSK>(mod, URHGPU_ERR_UNSUPPORTED, [&](auto m) {
//             hipLaunchKernelGGL((k_x<dt.value, m.value>), grid, block, 0, s, a);
//             return URHGPU_OK;
//         });
//     });
//
// A tag is an empty object: `dt.value` is the dtype code (what Iq<DT>, MagLoad<DT>, k_*<DT> take), `typename decltype(dt)::type` the element
// type (what the <T> launchers take); `m.value` the modulation (dispatch_mod is dispatch_one_of, which walks any set of integers);
// dispatch_bool hands std::true_type / std::false_type.  A site that has no
// instantiation for one of the values names none: `if constexpr (dt.value == URHGPU_DT_F32) return URHGPU_ERR_DTYPE; else { ... }`.
// The outer dispatch is the check that fires first where two could.
#pragma once
#include <stdint.h>

#include <tuple>
#include <type_traits>

#include "../../include/urhgpu.h"

namespace urh {

// code <-> element type: the one place that says so
using DtypeTypes = std::tuple<int8_t, uint8_t, int16_t, uint16_t, float>;
template <int DT>
struct DtypeTag : std::integral_constant<int, DT> {
    using type = std::tuple_element_t<DT, DtypeTypes>;
};
template <int DT, int BYTES, bool SIGNED, bool INTEGER = true>
constexpr bool dtype_is = sizeof(typename DtypeTag<DT>::type) == BYTES && std::is_signed<typename DtypeTag<DT>::type>::value == SIGNED &&
                          std::is_integral<typename DtypeTag<DT>::type>::value == INTEGER;
static_assert(dtype_is<URHGPU_DT_I8, 1, true>, "URHGPU_DT_I8 is int8_t");
static_assert(dtype_is<URHGPU_DT_U8, 1, false>, "URHGPU_DT_U8 is uint8_t");
static_assert(dtype_is<URHGPU_DT_I16, 2, true>, "URHGPU_DT_I16 is int16_t");
static_assert(dtype_is<URHGPU_DT_U16, 2, false>, "URHGPU_DT_U16 is uint16_t");
static_assert(dtype_is<URHGPU_DT_F32, 4, true, false>, "URHGPU_DT_F32 is float");

// f(DtypeTag) -> int for the five sample types; any other code: URHGPU_ERR_DTYPE
template <typename F>
int dispatch_dtype(int dtype, F &&f) {
    switch (dtype) {
        case URHGPU_DT_I8: return f(DtypeTag<URHGPU_DT_I8>{});
        case URHGPU_DT_U8: return f(DtypeTag<URHGPU_DT_U8>{});
        case URHGPU_DT_I16: return f(DtypeTag<URHGPU_DT_I16>{});
        case URHGPU_DT_U16: return f(DtypeTag<URHGPU_DT_U16>{});
        case URHGPU_DT_F32: return f(DtypeTag<URHGPU_DT_F32>{});
        default: return URHGPU_ERR_DTYPE;
    }
}

// f(std::integral_constant<int, V>) -> int for the one of VALUES... that v equals; none of them: `refused`, the site's own status.
// Any set of integers: the modulations a site accepts (kModGfsk among them), the Costas loop orders.
template <typename F>
int dispatch_one_of(int, int refused, F &&) {
    return refused;
}
template <int FIRST, int... REST, typename F>
int dispatch_one_of(int v, int refused, F &&f) {
    if (v == FIRST) return f(std::integral_constant<int, FIRST>{});
    return dispatch_one_of<REST...>(v, refused, f);
}
// ... under the name the modulation forks read best with
template <int... MODS, typename F>
int dispatch_mod(int mod, int refused, F &&f) {
    return dispatch_one_of<MODS...>(mod, refused, f);
}

// f(std::true_type) or f(std::false_type), whatever f returns: the order == 2, write_qad, d_noise != nullptr, loop_order == 4 forks
template <typename F>
decltype(auto) dispatch_bool(bool b, F &&f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

}  // namespace urh
