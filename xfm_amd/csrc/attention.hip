// Fused multi-head attention forward / backward for head_dim 64 (gfx950, bf16 MFMA, fp32 softmax): the host side.  The kernels live
// in one file per family (general: any shape; short: dense backward up to 256 keys; grouped: cross-attention per key/value source;
// vit: the 197-token batch walkers; long: dense backward at 577 / 901 tokens; aux: bias tiling, row fold, relative-position table),
// each with its shape predicate and its launches; this file checks the arguments, picks the route and runs it.
#include "attention_common.h"
#include "attention_general.hip"
#include "attention_short.hip"
#include "attention_grouped.hip"
#include "attention_vit.hip"
#include "attention_long.hip"
#include "attention_aux.hip"

static int attn_check(const AttnArgs& a, bool bwd) {
  XFM_REQUIRE(a.B > 0 && a.H > 0 && a.Sq > 0 && a.Sk > 0, "attention: empty problem B=%d H=%d Sq=%d Sk=%d", a.B, a.H, a.Sq, a.Sk);
  XFM_REQUIRE(a.q_rs % 8 == 0 && a.k_rs % 8 == 0 && a.v_rs % 8 == 0 && a.o_rs % 4 == 0, "attention: row strides must be multiples of 8");
  XFM_REQUIRE(((uintptr_t)a.q % 16) == 0 && ((uintptr_t)a.k % 16) == 0 && ((uintptr_t)a.v % 16) == 0 && ((uintptr_t)a.o % 8) == 0,
              "attention: q/k/v must be 16-byte aligned");
  XFM_REQUIRE(a.bias == nullptr || (a.bias_ld % 4 == 0 && a.bias_ld >= a.Sk), "attention: bias_ld must be a multiple of 4 and >= Sk");
  XFM_REQUIRE(a.B <= 65535 && a.H <= 65535, "attention: B/H exceed grid limits");
  XFM_REQUIRE(a.stat_ld >= a.Sq && a.stat_ld % 4 == 0 && ((uintptr_t)a.lse % 16) == 0, "attention: stat_ld must be a multiple of 4 and >= Sq, lse 16-byte aligned");
  XFM_REQUIRE(a.bias_t == nullptr || (a.bias != nullptr && a.bias_t_ld % 4 == 0 && a.bias_t_ld >= a.Sq), "attention: bad transposed bias");
  XFM_REQUIRE((a.q_start == nullptr) == (a.q_len == nullptr) && (a.k_start == nullptr) == (a.k_len == nullptr), "attention: packed rows need both start and len");
  XFM_REQUIRE((a.q_start == nullptr && a.k_start == nullptr) || (a.bias == nullptr && a.dbias == nullptr && a.kv_index == nullptr),
              "attention: packed rows take no additive bias and no kv_index");
  if (bwd) {
    XFM_REQUIRE(a.bwd_phase >= 0 && a.bwd_phase <= 2, "attention bwd: bwd_phase must be 0, 1 or 2");
    XFM_REQUIRE(a.dout && a.dq && a.dk && a.dv && a.delta && a.lse, "attention bwd: missing buffers");
    XFM_REQUIRE(a.do_rs % 8 == 0 && a.dq_rs % 4 == 0 && a.dk_rs % 4 == 0 && a.dv_rs % 4 == 0, "attention bwd: bad strides");
  }
  return XFM_OK;
}

static int attn_check_grouped(const AttnArgs& a) {
  XFM_REQUIRE(a.grp_rows != nullptr && a.n_groups > 0 && a.n_groups <= 65535, "grouped attention: grp_rows / n_groups missing");
  XFM_REQUIRE(a.Sq <= 64, "grouped attention needs Sq <= 64 (got %d)", a.Sq);   // (Sk > 256: the streamed-key kernels)
  XFM_REQUIRE(a.bias == nullptr && a.dbias == nullptr && a.causal == 0 && a.kv_index == nullptr,
              "grouped attention: no bias / causal mask / kv_index (the group index IS the key/value source)");
  // (the grouped kernels address source g's keys as rows g * Sk .. + Sk: a k_start / k_len pair would be ignored, not honoured)
  XFM_REQUIRE(a.k_start == nullptr && a.k_len == nullptr, "grouped attention: only the query side may be packed (k_start / k_len must be NULL)");
  return XFM_OK;
}

int xfm_attn_fwd_impl(const AttnArgs& a, hipStream_t st) {
  int rc = attn_check(a, false);
  if (rc != XFM_OK) return rc;
  if (a.grp_start != nullptr) {
    rc = attn_check_grouped(a);
    return rc != XFM_OK ? rc : launch_xattn_fwd(a, st);
  }
  if (attn_packable(a)) return launch_xattn_fwd_packed(a, st);
  if (attn_vit_shape(a)) return launch_attn_fwd_vit(a, st);
  return launch_attn_fwd(a, st);
}

// dbias[h, q, :] += sum_b ws[b, h, q, :]   (fp32, rows of ld floats; one thread per 4 columns, fixed summation order)
__global__ __launch_bounds__(256) void dbias_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dbias, int B, long per_entry) {
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= per_entry) return;
  f32x4 acc = *reinterpret_cast<const f32x4*>(dbias + e);
  for (int b = 0; b < B; ++b) acc += *reinterpret_cast<const f32x4*>(ws + (long)b * per_entry + e);
  *reinterpret_cast<f32x4*>(dbias + e) = acc;
}

// ---------------------------------------------------------------------------------------------
// The backward plan: which kernels one xfm_attn_bwd call runs and what they need, decided once from the arguments.  The
// dispatcher runs it and xfm_attn_bwd_workspace reports its `planes`, so the size of dbias_ws and the launches that write
// through it (with no size argument) cannot disagree.
// ---------------------------------------------------------------------------------------------
enum AttnDq { DQ_NONE, DQ_GROUPED, DQ_VIT, DQ_LONG, DQ_SHORT, DQ_SUMS, DQ_GENERAL };   // (grouped: resident or streamed by Sk; none: phase 2)
enum AttnDkv { DKV_NONE, DKV_GROUPED, DKV_LONG, DKV_SHORT, DKV_GENERAL };               // (none: phase 1, the ViT single pass)
// bias gradient: float atomics inside the dQ kernel | nb entries summed in registers (attn_bwd_dq_kernel<4, true, true>), then atomics |
// the general dQ kernel stores every entry's dS (B planes) | the short dQ kernel, one plane per batch slice (XFM_DETERMINISTIC=1) |
// attn_dbias_long_kernel after the dQ kernel: in place with one slice, else one plane per slice
enum AttnDbias { DB_NONE, DB_ATOMICS, DB_SUMS, DB_ENTRY_WS, DB_SHORT_PLANES, DB_BLOCKS };
struct AttnBwdPlan {
  AttnDq dq;
  AttnDkv dkv;
  AttnDbias dbias;
  int nw, blocks;          // general dQ kernel: waves per workgroup, query blocks
  int groups, nb, slices;  // short dQ kernel: query groups, batch entries per slice, slices; DQ_SUMS: nb; DB_BLOCKS: slices
  bool pre;                // short dQ kernel: delta from the forward's output
  int planes;              // [H, Sq, bias_ld] fp32 planes the route writes to dbias_ws and dbias_reduce_kernel folds into dbias (0: none)
};

// XFM_DETERMINISTIC=1: the reductions that still end in float atomics by default because the ordered form costs a launch or a pass
// (the bias gradient of the short attention backward: one plane per batch slice + dbias_reduce_kernel; the embedding gradients) take
// the ordered form.  Read per call.
static bool xfm_deterministic() { return xfm_env_flag("XFM_DETERMINISTIC", false); }

// have_ws: the caller offers a workspace (a.dbias_ws itself is not looked at).  Without one the short kernel falls back to atomics,
// the block kernel to one slice and the general kernel to per-element atomics.
static AttnBwdPlan attn_bwd_plan(const AttnArgs& a, bool have_ws) {
  AttnBwdPlan p = {};
  const bool run_dq = a.bwd_phase != 2, run_dkv = a.bwd_phase != 1;
  if (a.grp_start != nullptr) {   // (no bias gradient: attn_check_grouped)
    if (run_dq) p.dq = DQ_GROUPED;
    if (run_dkv) p.dkv = DKV_GROUPED;
    return p;
  }
  // the workspace routes store / sum 16-byte pieces of whole bias rows: every column of a row must lie in a key chunk the kernel visits
  const bool ws_ok = have_ws && a.dbias != nullptr && a.bias_ld % 4 == 0 && a.bias_ld <= (long)cdiv(a.Sk, 64) * 64 && a.q_start == nullptr;
  const int vit_mode = xfm_env_int("XFM_ATTN_VIT_BWD", 0);   // (read per call: the tests switch it inside one process)
  if (attn_vit3_shape(a, vit_mode)) {
    // opt-in single pass (dQ, dK, dV, delta in one kernel).  Mode 4 (experiment): WITHOUT its bias-gradient sums (they are what spills
    // it) + the block-walking bias-gradient kernel on the delta it wrote
    p.dq = DQ_VIT;
    if (a.dbias != nullptr) p.dbias = vit_mode == 4 && attn_dbias_blocks_ok(a) ? DB_BLOCKS : DB_ATOMICS;
  } else if (attn_long_shape(a)) {
    if (run_dq) {
      p.dq = DQ_LONG;
      if (a.dbias != nullptr) p.dbias = DB_BLOCKS;
    }
    if (run_dkv) p.dkv = attn_long_dkv_ok(a) ? DKV_LONG : DKV_GENERAL;
  } else {
    const bool short_ok = attn_short_dq_ok(a);
    attn_geom(a.Sq, p.nw, p.blocks);
    if (run_dq && short_ok) {
      p.dq = DQ_SHORT;
      p.slices = attn_short_dq_slices(a, p.groups, p.nb);
      p.pre = xfm_env_flag("XFM_ATTN_SHORT_PRE", false) && a.o != nullptr && a.o_lo != nullptr;   // (read per call, as above)
      if (a.dbias != nullptr) p.dbias = ws_ok && attn_short_planes_ok(a) && p.slices > 1 && xfm_deterministic() ? DB_SHORT_PLANES : DB_ATOMICS;
      if (p.dbias == DB_SHORT_PLANES) p.planes = p.slices;
    } else if (run_dq && a.dbias != nullptr && attn_resident(a.Sk, p.nw) && attn_plain(a)) {
      p.dq = DQ_SUMS;
      p.dbias = DB_SUMS;
      p.nb = attn_dbias_sums_nb(a, p.blocks);
    } else if (run_dq) {   // (a masked / causal / dropped problem with a bias gradient: per element)
      p.dq = DQ_GENERAL;
      // the workspace is for problems too long for the in-register sums; up to 256 keys the atomics stay
      if (a.dbias != nullptr) p.dbias = ws_ok && a.Sk > 64 * ATTN_RES_MAX ? DB_ENTRY_WS : DB_ATOMICS;
      if (p.dbias == DB_ENTRY_WS) p.planes = a.B;
    }
    if (run_dkv) p.dkv = short_ok && a.Sq <= 224 ? DKV_SHORT : DKV_GENERAL;
  }
  if (p.dbias == DB_BLOCKS) {
    p.slices = ws_ok ? attn_dbias_blocks_slices(a) : 1;   // (no plane buffer: one workgroup per block walks the whole batch)
    p.planes = p.slices > 1 ? p.slices : 0;
  }
  return p;
}

long xfm_attn_bwd_workspace_impl(const AttnArgs& a) { return (long)attn_bwd_plan(a, true).planes * a.H * a.Sq * a.bias_ld * 4; }

#ifdef XFM_DIAG
// Diagnostic build: where the next launches of attn_bwd_dq_short_kernel put their stamps (xfm_diag_set_timeline, capi.hip); ptr NULL = off
static XfmTimeline attn_short_timeline = {nullptr, 0, 0};
// the stamped build exists for the ViT shape only (tools/attn_timeline.py); every other launch of a diagnostic library goes unstamped
static long long* attn_short_stamps(const AttnArgs& a, unsigned workgroups) {
  long long* dbg = a.Sk > 128 && a.Sk <= 224 ? attn_short_timeline.ptr : nullptr;
  if (dbg != nullptr && attn_short_timeline.bytes < (size_t)workgroups * XFM_ATTN_SHORT_STAMP_BYTES) {
    xfm_set_error("attn_bwd_dq_short: timeline buffer of %zu bytes is short of %u workgroups x %d: launched without stamps",
                  attn_short_timeline.bytes, workgroups, XFM_ATTN_SHORT_STAMP_BYTES);
    dbg = nullptr;
  }
  return dbg == nullptr ? dbg : reinterpret_cast<long long*>((uintptr_t)dbg | (uintptr_t)(attn_short_timeline.flags & 15));
}
#endif

int xfm_attn_bwd_impl(const AttnArgs& a_in, hipStream_t st) {
  int rc = attn_check(a_in, true);
  if (rc == XFM_OK && a_in.grp_start != nullptr) rc = attn_check_grouped(a_in);
  if (rc != XFM_OK) return rc;
  const AttnBwdPlan p = attn_bwd_plan(a_in, a_in.dbias_ws != nullptr);
  AttnArgs a = a_in;
  if (p.planes == 0) a.dbias_ws = nullptr;   // the kernels take a non-NULL dbias_ws as "write the bias gradient there"

  switch (p.dq) {
    case DQ_NONE: break;   // dK/dV alone: `delta` was written by an earlier phase-1 call
    case DQ_GROUPED: rc = launch_xattn_dq(a, st); break;
    case DQ_VIT: {
      AttnArgs v = a;
      if (p.dbias == DB_BLOCKS) v.dbias = nullptr;
      rc = launch_attn_bwd_vit3(v, st);
      break;
    }
    case DQ_LONG: rc = launch_attn_bwd_long_dq(a, st); break;
    case DQ_SHORT:
#ifdef XFM_DIAG
      rc = launch_attn_bwd_dq_short(a, p.pre, p.groups, p.nb, p.slices, st, attn_short_stamps(a, (unsigned)(p.groups * a.H * p.slices)));
#else
      rc = launch_attn_bwd_dq_short(a, p.pre, p.groups, p.nb, p.slices, st);
#endif
      break;
    case DQ_SUMS: rc = launch_attn_bwd_dq(a, p.nw, p.blocks, p.nb, st); break;
    case DQ_GENERAL: rc = launch_attn_bwd_dq(a, p.nw, p.blocks, 0, st); break;
  }
  if (rc == XFM_OK && p.dbias == DB_BLOCKS) rc = launch_attn_dbias_blocks(a, p.slices, st);
  if (rc == XFM_OK && p.planes > 0) {   // the planes, in order
    const long per_entry = (long)a.H * a.Sq * a.bias_ld;
    hipLaunchKernelGGL(dbias_reduce_kernel, dim3(cdiv(per_entry / 4, 256)), dim3(256), 0, st, a.dbias_ws, a.dbias, p.planes, per_entry);
    rc = xfm_check_launch("dbias_reduce");
  }
  if (rc != XFM_OK) return rc;

  switch (p.dkv) {
    case DKV_NONE: break;
    case DKV_GROUPED: rc = launch_xattn_dkv(a, st); break;
    case DKV_LONG: rc = launch_attn_bwd_long_dkv(a, st); break;
    case DKV_SHORT: rc = launch_attn_bwd_dkv_short(a, st); break;
    case DKV_GENERAL: rc = launch_attn_bwd_dkv(a, st); break;
  }
  return rc;
}
