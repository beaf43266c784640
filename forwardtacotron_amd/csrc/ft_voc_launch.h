// The host side of the kernels of ft_voc_tile.h: the one width dispatch every vocoder launcher uses, and one launcher per
// shared kernel -- validation, grid and launch once, for both generators.  `who` is the caller's name in the messages
// ("melgan_conv_in", "hifigan_conv_in"); every limit and every grid is ft_voc_plan.h's.
#pragma once
#include <utility>

#include "ft_voc_tile.h"

namespace ft_voc_tile {

// f(PlanCfg<KIND, i>()) for the arrangement the plan picks for width c (the caller has checked that there is one)
template <int KIND, class F, int... I>
void with_cfg_at(int i, F& f, std::integer_sequence<int, I...>) {
  (void)((i == I && (f(PlanCfg<KIND, I>()), true)) || ...);
}
template <int KIND, class F>
void with_cfg(int c, F f) {
  with_cfg_at<KIND>(voc_plan::pick(KIND, c), f, std::make_integer_sequence<int, voc_plan::count(KIND)>());
}

inline dim3 grid_of(const voc_plan::Launch& g) { return dim3(g.x, g.y, g.z); }

// EDGE_REFLECT (MelGAN) adds the preconditions of a reflection by 3
template <int EDGE, bool NORM>
int launch_conv_in(const char* who, const float* mel, const long* lens, int B, int n_mels, int Tmax, int tail, float pad_value,
                   const float* w, const float* bias, int cout, float* out, int* err_flag, void* stream) {
  using namespace voc_plan;
  FT_REQUIRE(tile_rows(CONV_IN, n_mels) > 0, "%s: n_mels %d must be a multiple of 8 in 8..%d", who, n_mels, max_width(CONV_IN));
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && cout >= 1 && B <= MAX_BATCH, "%s: bad dims", who);
  if (EDGE == EDGE_REFLECT) {
    FT_REQUIRE(tail == 0 || tail >= REFLECT_MIN, "%s: a tail shorter than the reflection is not supported", who);
    FT_REQUIRE(tail + Tmax >= REFLECT_MIN, "%s: fewer than %d frames cannot be reflected by %d", who, REFLECT_MIN, IN_TAPS / 2);
  }
  FT_REQUIRE(mel && w && bias && out, "%s: null pointer", who);
  const Launch g = conv_in(B, Tmax, tail, n_mels, cout);
  with_cfg<CONV_IN>(n_mels, [&](auto cfg) {
    hipLaunchKernelGGL((conv_in_kernel<decltype(cfg), EDGE, NORM>), grid_of(g), dim3(g.threads), 0, (hipStream_t)stream, mel,
                       lens, Tmax, tail, pad_value, n_mels, w, bias, cout, g.cp, out, err_flag);
  });
  return ft_check_launch(who);
}

template <class Act>
int launch_upsample(const char* who, const float* x, const long* lens, int B, int Tmax, int tail, int scale, int cin, int cout,
                    int stride, const float* w, const float* bias, float* out, void* stream) {
  using namespace voc_plan;
  FT_REQUIRE(tile_rows(UPSAMPLE, cin) > 0, "%s: cin %d must be a multiple of 8 in 8..%d", who, cin, max_width(UPSAMPLE));
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && scale >= 1 && cout >= 1 && B <= MAX_BATCH, "%s: bad dims", who);
  FT_REQUIRE(stride_ok(stride), "%s: stride %d must be even (k = 2 stride, padding = stride / 2)", who, stride);
  FT_REQUIRE(x && w && bias && out && aligned16(x), "%s: null or misaligned pointer", who);
  const Launch g = upsample(B, Tmax, tail, scale, cin, cout, stride);
  with_cfg<UPSAMPLE>(cin, [&](auto cfg) {
    hipLaunchKernelGGL((upsample_kernel<decltype(cfg), Act>), grid_of(g), dim3(g.threads), 0, (hipStream_t)stream, x, lens,
                       Tmax, tail, scale, cin, cout, g.cp, stride, w, bias, out);
  });
  return ft_check_launch(who);
}

// EDGE_REFLECT (MelGAN): the shortest item, `scale` rows, must hold the reflection by 3
template <class Act, int EDGE>
int launch_conv_out(const char* who, const float* x, const long* lens, int B, int Tmax, int tail, int scale, int ch,
                    const float* w, float bias, float* wav, short* wav_i16, void* stream) {
  using namespace voc_plan;
  FT_REQUIRE(tile_rows(CONV_OUT, ch) > 0, "%s: %d channels must be a multiple of 8 in 8..%d", who, ch, max_width(CONV_OUT));
  FT_REQUIRE(B >= 1 && Tmax >= 1 && tail >= 0 && scale >= (EDGE == EDGE_REFLECT ? REFLECT_MIN : 1) && B <= MAX_BATCH,
             "%s: bad dims", who);
  FT_REQUIRE(x && w && wav && wav_i16 && aligned16(x), "%s: null or misaligned pointer", who);
  const Launch g = conv_out(B, Tmax, scale, ch);
  hipLaunchKernelGGL((conv_out_kernel<Act, EDGE>), grid_of(g), dim3(g.threads), 0, (hipStream_t)stream, x, lens, Tmax, tail,
                     scale, ch, w, bias, wav, wav_i16);
  return ft_check_launch(who);
}

}  // namespace ft_voc_tile
