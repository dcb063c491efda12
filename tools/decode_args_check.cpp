// Stand-alone host program for the argument checks of xfm_decode_attn, xfm_next_token and xfm_sample_token: every call below must be refused with XFM_E_ARG
// before anything is launched, so it runs without a GPU and touches no device memory (the non-NULL pointers are never read).  Meant for a
// host sanitizer build of the library's host code together with this file:
//   hipcc --offload-arch=gfx950 -O3 -g -std=c++17 -Xarch_host -fsanitize=address,undefined xfm_amd/csrc/capi.hip tools/decode_args_check.cpp
//         -o decode_args_check && ./decode_args_check
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../include/xfm_hip.h"

static int failures = 0;

static void expect_refused(const char* what, int rc, const char* word) {
  const char* msg = xfm_last_error();
  const bool ok = rc == XFM_E_ARG && strstr(msg, word) != nullptr;
  printf("%-44s rc=%d %s  [%s]\n", what, rc, ok ? "ok" : "UNEXPECTED", msg);
  if (!ok) ++failures;
}

static xfm_decode_attn_args attn_base() {
  xfm_bf16* p = reinterpret_cast<xfm_bf16*>(0x10000);   // 16-byte aligned, never dereferenced on the host
  xfm_decode_attn_args a;
  memset(&a, 0, sizeof(a));
  a.q = p; a.q_rs = 2304;
  a.k_new = p; a.k_new_rs = 2304;
  a.v_new = p; a.v_new_rs = 2304;
  a.k_cache = p; a.v_cache = p; a.rs = 1536;
  a.o = p; a.o_rs = 768;
  a.n_src = 2; a.B = 2; a.H = 12; a.cap = 8; a.pos = 3; a.Sk = 4; a.scale = 0.125f;
  return a;
}

static xfm_next_token_args token_base() {
  xfm_next_token_args a;
  memset(&a, 0, sizeof(a));
  a.logits = reinterpret_cast<const float*>(0x10000); a.ld = 64; a.V = 50;
  a.ids = reinterpret_cast<int64_t*>(0x10000); a.ids_ld = 9; a.cur_len = 3;
  a.penalty = 1.0f;
  a.unfinished = reinterpret_cast<int*>(0x10000);
  a.hist_unfinished = reinterpret_cast<int*>(0x10000);
  a.hist_logprob = reinterpret_cast<float*>(0x10000);
  a.hist_ld = 4; a.step = 1; a.pad_id = 1; a.n_eos = 1; a.eos_ids[0] = 2; a.B = 2;
  return a;
}

static xfm_sample_token_args sample_base() {
  xfm_sample_token_args a;
  memset(&a, 0, sizeof(a));
  a.logits = reinterpret_cast<const float*>(0x10000); a.ld = 64; a.V = 50;
  a.ids = reinterpret_cast<int64_t*>(0x10000); a.ids_ld = 9; a.cur_len = 3;
  a.penalty = 1.0f; a.temperature = 1.0f; a.top_k = 0; a.top_p = 1.0f;
  a.unfinished = reinterpret_cast<int*>(0x10000);
  a.hist_unfinished = reinterpret_cast<int*>(0x10000);
  a.hist_logprob = reinterpret_cast<float*>(0x10000);
  a.hist_ld = 4; a.step = 1; a.pad_id = 1; a.n_eos = 1; a.eos_ids[0] = 2; a.B = 2;
  return a;
}

int main() {
  expect_refused("decode_attn: NULL struct", xfm_decode_attn(nullptr, nullptr), "null");
  { auto a = attn_base(); a.pos = 8; a.Sk = 9; expect_refused("decode_attn: pos + 1 > cap", xfm_decode_attn(&a, nullptr), "capacity"); }
  { auto a = attn_base(); a.Sk = 5; expect_refused("decode_attn: Sk != pos + 1 (self)", xfm_decode_attn(&a, nullptr), "keys"); }
  { auto a = attn_base(); a.rs = 760; expect_refused("decode_attn: H * 64 > rs", xfm_decode_attn(&a, nullptr), "row stride"); }
  { auto a = attn_base(); a.k_new = nullptr; a.v_new = nullptr; a.Sk = 0; expect_refused("decode_attn: Sk < 1", xfm_decode_attn(&a, nullptr), "Sk"); }
  { auto a = attn_base(); a.k_new = nullptr; a.v_new = nullptr; a.Sk = 9; expect_refused("decode_attn: Sk > cap (cross)", xfm_decode_attn(&a, nullptr), "capacity"); }
  { auto a = attn_base(); a.v_new = nullptr; expect_refused("decode_attn: k_new without v_new", xfm_decode_attn(&a, nullptr), "v_new"); }
  { auto a = attn_base(); a.q = reinterpret_cast<xfm_bf16*>(0x10002); expect_refused("decode_attn: misaligned q", xfm_decode_attn(&a, nullptr), "16 bytes"); }
  { auto a = attn_base(); a.key_keep = reinterpret_cast<const int*>(0x10000); a.keep_ld = 3; expect_refused("decode_attn: keep_ld < Sk", xfm_decode_attn(&a, nullptr), "key_keep"); }
  { auto a = attn_base(); a.o = nullptr; expect_refused("decode_attn: NULL output", xfm_decode_attn(&a, nullptr), "null"); }

  expect_refused("next_token: NULL struct", xfm_next_token(nullptr, nullptr), "null");
  { auto a = token_base(); a.cur_len = 9; expect_refused("next_token: cur_len == ids_ld", xfm_next_token(&a, nullptr), "cur_len"); }
  { auto a = token_base(); a.cur_len = -1; expect_refused("next_token: cur_len < 0", xfm_next_token(&a, nullptr), "cur_len"); }
  { auto a = token_base(); a.step = 4; expect_refused("next_token: step == hist_ld", xfm_next_token(&a, nullptr), "step"); }
  { auto a = token_base(); a.V = 65; expect_refused("next_token: V > ld", xfm_next_token(&a, nullptr), "V="); }
  { auto a = token_base(); a.V = XFM_NEXT_TOKEN_MAX_V + 1; a.ld = a.V; expect_refused("next_token: V over the cap", xfm_next_token(&a, nullptr), "exceeds"); }
  { auto a = token_base(); a.n_eos = XFM_NEXT_TOKEN_MAX_EOS + 1; expect_refused("next_token: too many eos ids", xfm_next_token(&a, nullptr), "eos"); }
  { auto a = token_base(); a.penalty = 0.f; expect_refused("next_token: penalty 0", xfm_next_token(&a, nullptr), "penalty"); }
  { auto a = token_base(); a.ids = nullptr; expect_refused("next_token: NULL ids", xfm_next_token(&a, nullptr), "null"); }

  expect_refused("sample_token: NULL struct", xfm_sample_token(nullptr, nullptr), "null");
  { auto a = sample_base(); a.cur_len = 9; expect_refused("sample_token: cur_len == ids_ld", xfm_sample_token(&a, nullptr), "cur_len"); }
  { auto a = sample_base(); a.cur_len = -1; expect_refused("sample_token: cur_len < 0", xfm_sample_token(&a, nullptr), "cur_len"); }
  { auto a = sample_base(); a.step = 4; expect_refused("sample_token: step == hist_ld", xfm_sample_token(&a, nullptr), "step"); }
  { auto a = sample_base(); a.V = 65; expect_refused("sample_token: V > ld", xfm_sample_token(&a, nullptr), "V="); }
  { auto a = sample_base(); a.V = XFM_NEXT_TOKEN_MAX_V + 1; a.ld = a.V; expect_refused("sample_token: V over the cap", xfm_sample_token(&a, nullptr), "exceeds"); }
  { auto a = sample_base(); a.n_eos = XFM_NEXT_TOKEN_MAX_EOS + 1; expect_refused("sample_token: too many eos ids", xfm_sample_token(&a, nullptr), "eos"); }
  { auto a = sample_base(); a.penalty = 0.f; expect_refused("sample_token: penalty 0", xfm_sample_token(&a, nullptr), "penalty"); }
  { auto a = sample_base(); a.ids = nullptr; expect_refused("sample_token: NULL ids", xfm_sample_token(&a, nullptr), "null"); }
  { auto a = sample_base(); a.temperature = 0.f; expect_refused("sample_token: temperature 0", xfm_sample_token(&a, nullptr), "temperature"); }
  { auto a = sample_base(); a.temperature = -2.f; expect_refused("sample_token: temperature < 0", xfm_sample_token(&a, nullptr), "temperature"); }
  { auto a = sample_base(); a.temperature = INFINITY; expect_refused("sample_token: temperature inf", xfm_sample_token(&a, nullptr), "temperature"); }
  { auto a = sample_base(); a.temperature = NAN; expect_refused("sample_token: temperature NaN", xfm_sample_token(&a, nullptr), "temperature"); }
  { auto a = sample_base(); a.top_p = 0.f; expect_refused("sample_token: top_p 0", xfm_sample_token(&a, nullptr), "top_p"); }
  { auto a = sample_base(); a.top_p = 1.25f; expect_refused("sample_token: top_p > 1", xfm_sample_token(&a, nullptr), "top_p"); }
  { auto a = sample_base(); a.top_p = NAN; expect_refused("sample_token: top_p NaN", xfm_sample_token(&a, nullptr), "top_p"); }
  { auto a = sample_base(); a.top_k = -1; expect_refused("sample_token: top_k < 0", xfm_sample_token(&a, nullptr), "top_k"); }
  { auto a = sample_base(); a.filtered = reinterpret_cast<float*>(0x10000); a.filtered_ld = 49; expect_refused("sample_token: filtered_ld < V", xfm_sample_token(&a, nullptr), "filtered"); }
  printf("%s\n", failures == 0 ? "all refused as expected" : "FAILED");
  return failures == 0 ? 0 : 1;
}
