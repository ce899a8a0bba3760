// launch_dispatch.hpp -- run-time values to template arguments, once (host only): the padded widths the kernels
// are instantiated at, and the calls that pick one instantiation by width, by flag and by metric.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace kmx {

// a ladder of padded widths, ascending: what the host may choose (fit) is what the launchers instantiate (with_width)
template <int... Vs>
struct Widths {
  // the narrowest rung that holds D features; 0: none does
  static constexpr uint32_t fit(uint32_t D) {
    uint32_t dp = 0;
    ((dp == 0 && D <= (uint32_t)Vs ? void(dp = Vs) : void()), ...);
    return dp;
  }
  template <class F>
  static hipError_t call(uint32_t dp, F &&f) {
    hipError_t e = hipErrorInvalidValue;   // no such rung
    ((dp == (uint32_t)Vs ? void(e = f(std::integral_constant<int, Vs>{})) : void()), ...);
    return e;
  }
};
using FilterWidths = Widths<8, 16, 32, 64, 128, 256>;                  // the f32 filters (Lloyd, Yinyang, k-NN, predict)
using LloydF16Widths = Widths<16, 32, 64, 128, 256, 512>;              // the two-stage f16 Lloyd filter
using KnnF16Widths = Widths<16, 32, 64, 128, 256, 512, 768, 1024>;     // the f16 k-NN / radius filters
using HintWidths = Widths<16, 32, 64, 128, 256>;                       // the hinted Yinyang local filter

// f(std::integral_constant<int, V>{}) for the rung V == dp of ladder L; hipErrorInvalidValue without one
template <class L, class F>
hipError_t with_width(uint32_t dp, F &&f) { return L::call(dp, f); }
// f(std::true_type{}) or f(std::false_type{})
template <class F>
hipError_t with_flag(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// f(std::integral_constant<int, M>{}): M = 0 for the L2 metric, 1 otherwise (angular)
template <class F>
hipError_t with_metric(int metric, F &&f) {
  return metric == 0 ? f(std::integral_constant<int, 0>{}) : f(std::integral_constant<int, 1>{});
}

// 0: no MFMA filter instantiation, the exact kernels handle everything
inline uint32_t filter_dp_for(uint32_t D) { return FilterWidths::fit(D); }
// + 512 for 256 < D <= 512: the two-stage f16 Lloyd filter only
inline uint32_t lloyd_dp_for(uint32_t D) { return filter_dp_for(D) ? filter_dp_for(D) : LloydF16Widths::fit(D); }

}  // namespace kmx
