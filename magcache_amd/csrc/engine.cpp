// Host-side engine behind include/magcache_hip.h: weight store, workspace plan and the launch
// sequence of one DiT evaluation (the body of the reference's magcache_forward,
// MagCache4Wan2.1/magcache_generate.py:229-305) on a caller-supplied HIP stream.
//
// Nothing here allocates or synchronises during a forward: weights are converted once at
// mc_set_weight, all scratch + the residual cache are carved from one caller-owned workspace, the
// MagCache decision is made by the caller on the host (reference :277-292 never touches the GPU).
#include <cmath>
#include <cstddef>
#include <memory>

#include "host.h"

using mc::align_up;
using mc::bf16_t;
using mc::fail;
using mc::Keys;
using mc::Linear;
using mc::RowRange;
using mc::whole;

namespace {

struct Layer {
  Linear qkv, o, cq, ckv, co, ffn1, ffn2;   // self-attention q|k|v and o, cross-attention q, k|v and o, the FFN
  float *nq, *nk, *cnq, *cnk, *n3w, *n3b, *mod;
  Linear ckv_img;  // I2V: [k_img ; v_img]
  float* cnk_img = nullptr;
  int index = 0;   // flat: main layers 0 .. NL-1, then the VACE blocks (the order of "emod" and "ckv_cache")
};

}  // namespace

constexpr int kSpMaxParts = 9;   // local shard + 8 gather rounds

struct mc_engine {
  mc_config cfg;
  mc::MxFormat mx_fmt = mc::MX_E4M3;   // the element format of the MX Linears (fp8_linear 2 | 3), as mc_create latched it from the
                                       // options "mx_fp4" / "mx_fp6" (host.h: latch_mx_format)
  int d, ffn, H, NL, L, Lr, Lp, P, rank, tok0, Kp;  // Kp = in_dim*4 padded to 64
  int ctx_rows;                                     // text_len padded to 64
  std::vector<Layer> layers;
  // non-block weights: the Linears of the embeds; the time MLP and the head are fp32 (gemv_f32 / head_linear)
  Linear patch, text0, text1;
  float *w_time0, *b_time0, *w_time1, *b_time1, *w_tproj, *b_tproj;
  float *w_head, *b_head, *head_mod;
  // I2V img_emb = MLPProj(clip_dim -> dim): LayerNorm, Linear, GELU, Linear, LayerNorm
  Linear img1, img3;
  float *ln_img0_w = nullptr, *ln_img0_b = nullptr, *ln_img4_w = nullptr, *ln_img4_b = nullptr;
  int img_rows = 0;     // 257 image tokens padded to a multiple of 64
  bool have_clip = false;
  // sequence parallel (P > 1): the gathered K|V of a layer arrive in sp_chunks rounds (mc_sp_set_chunks); the self-attention
  // of a layer is a chain of launches merged by their log2-sum-exp: [this rank's shard] + one launch per round
  bool sp = false;             // sp_size > 1, or sp_phases: the phase path with its buffers on a world of one
  int sp_chunks = 1;
  int attn_layer = -2;         // whose attention chain is open: main layer >= 0, a VACE block -1, none -2
  int attn_launches = 0;       // launches of that chain so far ("ao" / "attn_lse" hold their merged result)
  bool attn_local_done = false;
  int attn_rounds_done = 0;
  // mc_blocks_sp with sp_attn_partials (default): the launches of a chain run independently on `stream` and this side
  // stream, each into its own slot of "ao_part" / "lse_part", and attn_merge joins them
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  size_t splitk_bytes = 0;     // "splitk": scratch for FFN-2's split-K where a rank's shard leaves the chip under-filled
  // text context cache (mc_set_context): per slot the embedded context and every block's normalised cross-attention
  // K|V; a forward called with context_dev == NULL reads slot ctx_active instead of recomputing them
  bool ctx_valid[2] = {false, false};
  int ctx_active = -1;
  const float* tok_t = nullptr;  // Wan2.2 TI2V: per-token timesteps of the next forwards (mc_set_token_timesteps)
  int HT = 64;                   // row stride of "head_tokens": 4*out_dim rounded up to 64
  // optional in-stream timing: hipEvent pairs around the launches of a forward, tagged with a class (mc_prof_class).
  // level 1 = the dominant kernel only (self-attention), level 2 = every launch of a block + embed / head
  int profile = 0;
  std::vector<hipEvent_t> prof_ev;
  std::vector<uint8_t> prof_cls;   // class of pair i (events 2 i, 2 i + 1)
  size_t prof_n = 0;  // events used
  // VACE (upstream wan/modules/vace_model.py VaceWanModel): n_vace extra blocks on a control stream c; block i feeds
  // main layer i * vace_stride through after_proj ("hint")
  std::vector<Layer> vlayers;
  Linear vpatch, before;
  std::vector<Linear> after;
  float* vscale = nullptr;
  int NV = 0, Kvp = 0;
  bool have_vace = false;
  float* cs_table = nullptr;  // rope (cos,sin) [Lp][64][2]: expanded on the device from the per-axis values in rope_axes
  float* rope_axes = nullptr; // (cos,sin) pairs of the grid's frame, height and width positions (mc_op_rope_axes layout)
  int cs_rows = 0;            // rows allocated behind cs_table (>= Lp: mc_set_geometry grows it, never shrinks it)
  size_t axes_cap = 0;        // floats allocated behind rope_axes
  bool phase_open = false;    // between mc_embed and mc_head of a phase forward (mc_set_geometry refuses)
  mc::WeightStore weights;
  mc::Workspace work;
  int res_slot[2] = {0, 1};  // residual buffer index held by branch b
  int res_scratch = 2;
  bool have_res[2] = {false, false};
  bool have_stats[2] = {false, false};
  bool embedded = false;
  // CFG pair (mc_pair_begin / mc_pair_end): the caller has declared that the next two mc_forward calls receive the same
  // latent and the same t.  The first one that runs its blocks keeps the context-free front of the evaluation -- the embeds
  // of the latent and of t, and layer 0 up to its normalised cross-attention q -- and the second continues from it:
  // "pair_x" = the fp32 stream after layer 0's O epilogue, "pair_cq" = the cross-attention q rows; "x0", "emod", "ehead"
  // and "tok_sel" are written by the embeds only and survive as they are.
  enum { PAIR_NONE, PAIR_ARMED, PAIR_KEPT, PAIR_DEAD };
  int pair = PAIR_NONE;
  const float *pair_latent = nullptr, *pair_t_dev = nullptr;   // what the kept front was computed from
  double pair_t_host = 0.0;
  // sharded, VACE, I2V and fp8 engines never share: they run every forward in full
  bool pair_capable() const { return !sp && NV == 0 && cfg.clip_dim == 0 && cfg.fp8_linear == 0; }
  void pair_drop() { if (pair != PAIR_NONE) pair = PAIR_DEAD; }   // forget a kept front; the pair runs in full from here

  template <class T>
  T* buf(const char* name) const { return work.get<T>(name); }
  float* residual(int idx) const {
    static const char* names[3] = {"residual0", "residual1", "residual2"};
    return buf<float>(names[idx]);
  }
  // main or VACE layer by flat index, and the 6 modulation vectors of a layer (set 0; second_set() for the other)
  const Layer& layer(int flat) const { return flat < NL ? layers[flat] : vlayers[flat - NL]; }
  const float* emod(const Layer& l) const { return buf<float>("emod") + (size_t)l.index * 6 * d; }
};

namespace {

// Measurement hook (mc_profile_enable): one hipEvent pair on the launch stream around the launches of the enclosing
// scope, tagged with its class.  Level 1 brackets the self-attention launches only (what bench.py's timed region carries),
// level 2 every class.  The pair is reserved at construction, so scopes may nest.  A failed record is not an error of
// the forward: the pair is dropped from the log.  A negative class logs nothing.
struct Prof {
  mc_engine* e;
  hipStream_t s;
  size_t idx = 0;
  bool on = false;
  Prof(mc_engine* e_, int cls, hipStream_t s_) : e(e_), s(s_) {
    if (cls < 0 || !e->profile || (e->profile < 2 && cls != MC_PROF_ATTN_SELF) || e->prof_n + 2 > e->prof_ev.size()) return;
    idx = e->prof_n;
    if (hipEventRecord(e->prof_ev[idx], s) != hipSuccess) return;
    e->prof_cls[idx / 2] = (uint8_t)cls;
    e->prof_n += 2;
    on = true;
  }
  ~Prof() {
    if (on && hipEventRecord(e->prof_ev[idx + 1], s) != hipSuccess) e->prof_cls[idx / 2] = 0xff;
  }
  Prof(const Prof&) = delete;
  Prof& operator=(const Prof&) = delete;
};

// upstream rope_params / rope_apply frequency split for head_dim 128 (22 + 21 + 21 complex pairs)
constexpr int kRopeT = mc::kRopePairsT, kRopeHW = mc::kRopePairsHW;
constexpr double kRopeDimT = 44.0, kRopeDimHW = 42.0;   // d - 4 * (d / 6), 2 * (d / 6)

// THE per-entry expression: (cos, sin) of position `pos` on an axis, frequency j of the axis' `dim` rotary channels.  The
// per-token table (rope_table_host) and the per-axis values (rope_axes_host) both come from here, so that the table the
// device expands from the axes is the host table bit for bit.
inline void rope_pair(int pos, int j, double dim, float* cs) {
  const double fr = 1.0 / std::pow(10000.0, (2.0 * j) / dim);
  const double a = (double)pos * fr;
  cs[0] = (float)std::cos(a);
  cs[1] = (float)std::sin(a);
}

void rope_table_host(int F, int Hp, int Wp, int tok0, int n_tok, float* cs) {
  const int c = kRopeT + 2 * kRopeHW;
  for (int r = 0; r < n_tok; ++r) {
    const int tok = tok0 + r;
    float* row = cs + (size_t)r * 2 * c;
    if (tok >= F * Hp * Wp) {  // padded token: identity rotation (upstream leaves the tail untouched)
      for (int i = 0; i < c; ++i) { row[2 * i] = 1.f; row[2 * i + 1] = 0.f; }
      continue;
    }
    const int f = tok / (Hp * Wp), rem = tok % (Hp * Wp), h = rem / Wp, w = rem % Wp;
    for (int i = 0; i < c; ++i) {
      if (i < kRopeT) rope_pair(f, i, kRopeDimT, row + 2 * i);
      else if (i < kRopeT + kRopeHW) rope_pair(h, i - kRopeT, kRopeDimHW, row + 2 * i);
      else rope_pair(w, i - kRopeT - kRopeHW, kRopeDimHW, row + 2 * i);
    }
  }
}

// what the table is separable into: entry (token, i) depends on ONE of the token's grid coordinates.  F x 22 pairs of the
// frame axis, then Hp x 21 of the height axis, then Wp x 21 of the width axis
size_t rope_axes_floats(int F, int Hp, int Wp) { return 2 * ((size_t)F * kRopeT + ((size_t)Hp + Wp) * kRopeHW); }

void rope_axes_host(int F, int Hp, int Wp, float* axes) {
  for (int f = 0; f < F; ++f)
    for (int j = 0; j < kRopeT; ++j, axes += 2) rope_pair(f, j, kRopeDimT, axes);
  for (int h = 0; h < Hp; ++h)
    for (int j = 0; j < kRopeHW; ++j, axes += 2) rope_pair(h, j, kRopeDimHW, axes);
  for (int w = 0; w < Wp; ++w)
    for (int j = 0; j < kRopeHW; ++j, axes += 2) rope_pair(w, j, kRopeDimHW, axes);
}

// ---- the latent grid: what a call may change (mc_set_geometry).  mc_create and mc_set_geometry share all of it.
struct Rows { int L, Lr, Lp, tok0; };   // tokens of the sequence, of this rank, padded to the attention tile, first global token

mc_status check_geometry(int latent_f, int latent_h, int latent_w, int P) {
  if ((latent_h & 1) || (latent_w & 1) || latent_f <= 0 || latent_h <= 0 || latent_w <= 0)
    return fail(MC_EINVAL, "latent grid %dx%dx%d not divisible by patch (1,2,2)", latent_f, latent_h, latent_w);
  const long long L = (long long)latent_f * (latent_h / 2) * (latent_w / 2);
  if (L > (1ll << 24)) return fail(MC_EINVAL, "latent grid %dx%dx%d: %lld tokens", latent_f, latent_h, latent_w, L);
  if (L % P) return fail(MC_EINVAL, "seq_len %d not divisible by sp_size %d", (int)L, P);
  return MC_OK;
}

Rows derive_rows(int latent_f, int latent_h, int latent_w, int P, int rank) {
  Rows r;
  r.L = latent_f * (latent_h / 2) * (latent_w / 2);
  r.Lr = r.L / P;
  r.Lp = (int)align_up(r.Lr, 256);
  r.tok0 = rank * r.Lr;
  return r;
}

// split-K scratch of FFN-2 (K = ffn): a rank of a wide sequence-parallel job has too few 256^2 tiles for the chip (sp 8 at
// 1.3B: M = 4096 -> 96 tiles), launch_gemm_bf16 then cuts K in slices (policy: gemm_bf16_v2.hip); 0 bytes where it would not
size_t splitk_need(const mc_engine* e, int Lp) {
  return e->sp ? mc::gemm_splitk_ws_need(Lp, e->d, e->ffn, mc::EPI_RESID_GATE) : 0;
}

void plan_workspace(const mc_engine* e, const Rows& rows, mc::Workspace& ws) {
  const mc_config& c = e->cfg;
  const size_t d = e->d, ffn = e->ffn;
  const size_t Lp = rows.Lp;
  ws.add("x", Lp * d * 4);
  ws.add("x0", Lp * d * 2);
  ws.add("xn", Lp * d * 2);
  ws.add("qkv", Lp * 3 * d * 2);  // P>1: only the first Lp*d (q) is used
  ws.add("ao", Lp * d * 2);
  ws.add("h", std::max(Lp * ffn * 2, Lp * d * 4));  // FFN hidden (bf16) / head LN out (fp32)
  ws.add("tokens", Lp * e->Kp * 2);
  ws.add("ctx_in", (size_t)e->ctx_rows * c.text_dim * 2);
  ws.add("ctx_h", (size_t)e->ctx_rows * d * 2);
  ws.add("ctx", (size_t)e->ctx_rows * d * 2);
  ws.add("ckv", (size_t)e->ctx_rows * 2 * d * 2);
  ws.add("ctx_cache", (size_t)2 * e->ctx_rows * d * 2);                              // [2 slots][ctx_rows][d]
  if (!c.no_context_cache)      // (0.84 GB at 14B that a caller who passes its context every forward never uses)
    ws.add("ckv_cache", (size_t)2 * (e->NL + e->NV) * e->ctx_rows * 2 * d * 2);      // [2][layers][ctx_rows][2d]
  // two sets of everything that depends on t: set 0 for the (maximum) timestep, set 1 for the second value per-token
  // timesteps may carry (Wan2.2 TI2V: the conditioning frame's tokens have t = 0)
  // token_timestep_sets = C: C sets at the same per-set strides, one per distinct per-token timestep ("tok_vals": the values)
  const size_t tsets = c.no_token_timesteps ? 1 : c.token_timestep_sets ? (size_t)c.token_timestep_sets : 2;
  ws.add("temb", tsets * (c.freq_dim + 2 * d + 6 * d) * 4);  // sets x (sinus | h1 | e | e0)
  ws.add("emod", tsets * (e->NL + e->NV) * 6 * d * 4);
  ws.add("tok_sel", c.no_token_timesteps ? 256 : (size_t)Lp + 256);
  ws.add("tok_t2", 64);
  if (c.fp8_linear) {
    ws.add("aq", Lp * std::max(d, ffn));            // e4m3 activations of the current fp8 GEMM
    ws.add("a_scale", Lp * 4);                      // their per-token scales
    if (c.fp8_linear >= 2) ws.add("a_mx", (std::max(d, ffn) / 32) * Lp);   // MX: per (token, 32 k) block scales
  }
  if (e->NV > 0) {
    ws.add("xc", Lp * d * 4);                       // VACE control stream c (fp32 like x)
    ws.add("c0", Lp * d * 2);                       // vace_patch_embedding(vace_context), constant per video
    ws.add("vtokens", Lp * (size_t)e->Kvp * 2);
  }
  ws.add("ehead", std::max<size_t>(2, tsets) * 2 * d * 4);
  ws.add("head_tokens", (size_t)Lp * e->HT * 4);
  // sequence parallel: "kv_local" [Lp][2d] = this rank's post-norm, post-RoPE K|V rows (the send buffer of the gather);
  // "kv_gather" [C][P][Lp / C][2d] = round c of the gather holds rows [c Lp / C, (c + 1) Lp / C) of EVERY rank's shard
  ws.add("kv_local", e->sp ? Lp * 2 * d * 2 : 256);
  ws.add("kv_gather", e->sp ? (size_t)e->P * Lp * 2 * d * 2 : 256);
  ws.add("residual0", Lp * d * 4);
  ws.add("residual1", c.n_branches > 1 ? Lp * d * 4 : 256);
  ws.add("residual2", c.calibration ? Lp * d * 4 : 256);
  if (c.clip_dim > 0) {
    const size_t ir = e->img_rows, cd = c.clip_dim;
    ws.add("clip_in", ir * cd * 4);
    ws.add("clip_n", ir * cd * 2);
    ws.add("clip_h", ir * cd * 2);
    ws.add("clip_o", ir * d * 4);
    ws.add("clip_h2", ir * d * 2);
    ws.add("ctx_img", ir * d * 2);
    ws.add("ckv_img", ir * 2 * d * 2);
    ws.add("ao2", Lp * d * 2);
  }
  if (e->sp) ws.add("attn_lse", (size_t)e->H * Lp * 4);
  const size_t splitk = splitk_need(e, rows.Lp);     // split-K scratch of FFN-2
  ws.add("splitk", splitk ? splitk : 256);
  // partial attention results of a layer's chain (local shard + up to 8 gather rounds), merged by attn_merge
  ws.add("ao_part", e->P > 1 ? (size_t)kSpMaxParts * Lp * d * 2 : 256);
  ws.add("lse_part", e->P > 1 ? (size_t)kSpMaxParts * e->H * Lp * 4 : 256);
  ws.add("calib_partial", (2048 * 4 + 2) * 8);   // + the arrival ticket of calib_stats_kernel
  ws.add("calib_sums", 4 * 8);
  ws.add("calib_stats", 2 * 3 * 4);
  // the kept front of a CFG pair (mc_pair_begin): last in the plan, every other offset stays where it was
  ws.add("pair_x", e->pair_capable() ? Lp * d * 4 : 256);
  ws.add("pair_cq", e->pair_capable() ? Lp * d * 2 : 256);
  if (c.token_timestep_sets) ws.add("tok_vals", 256);   // (behind the kept front: a default engine's plan is what it was)
}

// The RoPE table of the engine's grid, for this rank's rows: the per-axis values are computed on the host (the doubles of
// rope_table_host), uploaded -- a few tens of KB -- and expanded to [Lp][64][2] by one launch; rows >= Lr are padding:
// identity.  rope_reserve is the one step that allocates (through the weight store, never inside a forward), so that
// mc_set_geometry can run it before anything changes.
mc_status rope_reserve(mc_engine* e, int Lp, size_t axes_floats) {
  if (Lp > e->cs_rows) {
    float* grown = nullptr;
    MC_TRY(e->weights.alloc(&grown, (size_t)Lp * 128));
    if (e->cs_table) e->weights.release(e->cs_table);
    e->cs_table = grown;
    e->cs_rows = Lp;
  }
  if (axes_floats > e->axes_cap) {
    float* grown = nullptr;
    MC_TRY(e->weights.alloc(&grown, axes_floats));
    if (e->rope_axes) e->weights.release(e->rope_axes);
    e->rope_axes = grown;
    e->axes_cap = axes_floats;
  }
  return MC_OK;
}

mc_status rope_build(mc_engine* e) {
  const int F = e->cfg.latent_f, Hp = e->cfg.latent_h / 2, Wp = e->cfg.latent_w / 2;
  std::vector<float> axes(rope_axes_floats(F, Hp, Wp));
  rope_axes_host(F, Hp, Wp, axes.data());
  HIP_TRY(hipMemcpy(e->rope_axes, axes.data(), axes.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(mc::launch_rope_expand(e->rope_axes, F, Hp, Wp, e->tok0, e->Lr, e->Lp, e->cs_table, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));   // the forwards run on the caller's streams
  return MC_OK;
}

// What a (re)bound or re-planned workspace means for the state: everything that lived at an offset that may have moved, or in
// memory that is no longer the engine's, is forgotten -- the residual caches and calibration statistics, the embeds of an
// open phase forward, both text-context slots, the CLIP image context, the VACE context and a kept CFG front; per-token
// timesteps were a vector over the old sequence.  (Before 0.7 mc_set_workspace kept ctx_valid, have_clip and have_vace, whose
// bytes a rebind loses as surely as a re-plan does; no caller could tell: the Python shim binds once, before any of them is set.)
mc_status forget_workspace_state(mc_engine* e) {
  e->have_res[0] = e->have_res[1] = false;
  e->have_stats[0] = e->have_stats[1] = false;
  e->res_slot[0] = 0; e->res_slot[1] = 1; e->res_scratch = 2;
  e->embedded = e->phase_open = false;
  e->ctx_valid[0] = e->ctx_valid[1] = false;
  e->ctx_active = -1;
  e->have_clip = e->have_vace = false;
  e->tok_t = nullptr;
  e->attn_layer = -2;
  e->pair_drop();
  // the arrival ticket of the one-launch calibration reduction starts at zero (the kernel rearms it itself)
  if (e->work.ws) HIP_TRY(hipMemset(e->buf<double>("calib_partial") + 2048 * 4, 0, 16));
  return MC_OK;
}

mc_status check_ready(const mc_engine* e) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->weights.dirty()) return fail(MC_ESTATE, "LoRA adapters, scales or a touched weight changed: call mc_lora_apply first");
  return mc::check_ready(e->work, e->weights, "mc_set_workspace");
}

// ---- the one launch path of the engine's Linears
// The activation rows [M, k_in] a Linear reads.  A bf16 Linear reads `rows`.  An fp8 Linear reads e4m3 rows + scales:
// it quantises `rows` into "aq" (+ "a_scale" | "a_mx") first, unless they are `quantised` already -- there by a fused producer
// or an earlier Linear over the same rows, or, q / mx given, in the caller's buffers (FFN-1's GELU epilogue writes FFN-2's).
struct ActSrc {
  const bf16_t* rows = nullptr; long ld = 0;
  bool quantised = false;
  uint8_t *q = nullptr, *mx = nullptr;
};

// Does a fused producer (the LayerNorm tail, FFN-1's GELU epilogue) write the quantised rows this Linear reads?  With
// fp8_fused_quant, for the per-row and the e4m3 MX copies; this engine has no fused producer of e2m1 or e2m3 rows: the separate pass.
bool fused_quant(const Linear& l) { return l.q && mc::g_fp8_fused_quant && (!l.mx || l.fmt == mc::MX_E4M3); }

// y[:, out] = epilogue(a W[out]^T + b[out]) over M rows: p carries the outputs, gates, capture and split-K operands of the
// epilogue; the operands, the shape and every pointer advance of a row range come from `l`.
// fp8 (block Linears only, M = Lp: "aq" and its scales are planned for that): per-token activation scales x per-output-channel
// weight scales (launch_gemm_fp8), or MX block scales on both sides -- activations per (token, 32 k), weights per
// (channel, 32 k), in the Linear's element format -- multiplied inside the matrix core (launch_gemm_mx).
mc_status linear(mc_engine* e, const Linear& l, RowRange out, int M, ActSrc a, mc::GemmParams p, int epi, hipStream_t s) {
  const int K = l.k_in;
  if (!l.q) {
    HIP_TRY(mc::launch_linear_bf16(l, out, a.rows, a.ld, M, p, epi, s));
    return MC_OK;
  }
  const int Lp = e->Lp;
  if (M != Lp) return fail(MC_EINVAL, "an fp8 Linear runs over the %d rows of a block, not %d", Lp, M);
  p.M = Lp; p.N = out.count; p.K = K; p.bias = l.b + out.first;
  uint8_t* aq = a.q ? a.q : e->buf<uint8_t>("aq");
  if (l.mx) {   // packed rows of q_row_bytes on both sides, block-major scale images: [k / 32][rows]
    const long kb = l.q_row_bytes();
    uint8_t* am = a.mx ? a.mx : e->buf<uint8_t>("a_mx");
    if (!a.quantised) HIP_TRY(mc::launch_quantize_rows_mx(l.fmt, a.rows, nullptr, a.ld, Lp, K, aq, kb, am, (long)Lp, s));
    p.A = (const bf16_t*)aq; p.lda = kb; p.W = (const bf16_t*)(l.q + (size_t)out.first * kb); p.ldw = kb;
    p.a_mx = am; p.mx_rows_a = (long)Lp; p.w_mx = l.mx + out.first; p.mx_rows_w = l.n_out;
    HIP_TRY(mc::launch_gemm_mx(l.fmt, p, epi, s));
    return MC_OK;
  }
  p.A = (const bf16_t*)aq; p.lda = K; p.W = (const bf16_t*)(l.q + (size_t)out.first * K); p.ldw = K;
  float* as = e->buf<float>("a_scale");
  if (!a.quantised) HIP_TRY(mc::launch_quantize_rows_fp8(a.rows, nullptr, a.ld, Lp, K, aq, K, as, s));
  p.a_scale = as; p.w_scale = l.q_scale + out.first;
  HIP_TRY(mc::launch_gemm_fp8(p, epi, s));
  return MC_OK;
}
// the common case: every output channel into a bf16 matrix C (ld = n_out)
mc_status linear_bf16_out(mc_engine* e, const Linear& l, int M, ActSrc a, bf16_t* C, int epi, hipStream_t s) {
  mc::GemmParams p = {};
  p.Cb = C; p.ldc = l.n_out;
  return linear(e, l, whole(l), M, a, p, epi, s);
}

// ---- the key sets of the engine's attention launches (mc::Keys) and the one launch over them
Keys kv_pairs(const bf16_t* kv, int d, int rows, int valid) { return {kv, kv + d, 2L * d, 0, rows, valid, 1, 0}; }   // rows of [k | v]
Keys qkv_keys(const mc_engine* e) {   // one device: the k and v columns of "qkv"
  const bf16_t* k = e->buf<bf16_t>("qkv") + e->d;
  return {k, k + e->d, 3L * e->d, 0, e->Lp, e->Lr, 1, 0};
}
Keys local_keys(const mc_engine* e) { return kv_pairs(e->buf<bf16_t>("kv_local"), e->d, e->Lp, e->Lr); }   // this rank's shard
// sequence-parallel geometry of the gather rounds (mc_sp_set_chunks)
int sp_chunk_rows(const mc_engine* e) { return e->Lp / e->sp_chunks; }
int sp_round_valid(const mc_engine* e, int c) {   // valid keys at the start of every shard's chunk c
  const int lc = sp_chunk_rows(e);
  return std::max(0, std::min(lc, e->Lr - c * lc));
}
int sp_rounds(const mc_engine* e) {               // rounds that carry at least one valid key
  const int lc = sp_chunk_rows(e);
  return (e->Lr + lc - 1) / lc;
}
// round < 0: this rank's own shard; round c: "kv_gather"[c] = [P][Lp / C][2d], with or without this rank's shard
Keys sp_keys(const mc_engine* e, int round, bool skip_own) {
  if (round < 0) return local_keys(e);
  const int lc = sp_chunk_rows(e), d = e->d;
  Keys k = kv_pairs(e->buf<bf16_t>("kv_gather") + (size_t)round * e->P * lc * 2 * d, d, lc, sp_round_valid(e, round));
  k.stride = (long)lc * 2 * d; k.n_shards = e->P; k.skip_shard_p1 = skip_own ? e->rank + 1 : 0;
  return k;
}
// the Lp query rows of Q over one key set -> O [Lp][d]
mc_status attend(const mc_engine* e, const bf16_t* Q, long ldq, bf16_t* O, const Keys& keys, const float* lse_in, float* lse_out,
                 hipStream_t s) {
  HIP_TRY(mc::launch_attention_keys(Q, ldq, O, e->d, e->Lp, e->H, keys, lse_in, lse_out, s));
  return MC_OK;
}
// whose self-attention chain is open and how far it got (sequence parallel)
void attn_chain_set(mc_engine* e, int layer, int launches, bool local_done, int rounds_done) {
  e->attn_layer = layer; e->attn_launches = launches; e->attn_local_done = local_done; e->attn_rounds_done = rounds_done;
}
void attn_chain_open(mc_engine* e, int layer) {
  if (e->attn_layer != layer) attn_chain_set(e, layer, 0, false, 0);
}

}  // namespace

namespace mc {
// option "fp8_fused_quant" (0 | 1): 1 (default) = with fp8_linear the LayerNorm + modulate kernel (and, MX, the GELU
// epilogue of FFN-1) write the e4m3 operand of the next GEMM directly; 0 = round 3's separate quantise passes (same bits).
int g_fp8_fused_quant = 1;
// option "sp_attn_partials" (0 | 1 | 2): mc_blocks_sp runs the launches of a layer's self-attention chain independently on
// two streams into partial buffers + one merge kernel -- 1 (default) when a rank's launch fills less than 90 % of the CU slots
// of the waves it runs in (query blocks x heads against the CU count: 384 workgroups at sp 4 and 192 at sp 8 are 75 %; sp 2's
// 768 are 100 % and 14B's 1480 at sp 8 96 %: there the merge only costs -- measured -4 % / -4 % / +2 % / +3 % of the layer loop
// at 1.3B sp 4 / 8 / 2 and 14B sp 8, profiles/r06/sp_timeline*.log), 2 always, 0 never
// (one stream, merged in place launch by launch)
int g_sp_attn_partials = 1;
// option "mx_fp4" (0 | 1): read once by mc_create; 1 with fp8_linear 2 | 3 = the MX Linears hold an MXFP4 copy (W4A4,
// gemm_mxfp4.hip) and their activations are quantised by separate passes.  The engine keeps what it read (mc_engine::mx_fmt).
int g_mx_fp4 = 0;
// option "mx_fp6" (0 | 1): the same latch for MXFP6 copies (W6A6, gemm_mxfp6.hip); a create call that finds both at 1 is refused
int g_mx_fp6 = 0;
}  // namespace mc
static int g_n_cu = 0;

extern "C" {

// mc_config only ever grows at its END, and a zero in a new field keeps the behaviour older callers had: a caller built
// against an older header passes ITS sizeof(mc_config) and the tail reads as zeros (instead of being read past the end of
// the caller's struct, as mc_create would)
mc_status mc_create_sized(const mc_config* cfg, size_t cfg_bytes, mc_engine** out) {
  if (!cfg || !out) return fail(MC_EINVAL, "null argument");
  if (cfg_bytes < offsetof(mc_config, fp8_linear) || cfg_bytes > sizeof(mc_config) || (cfg_bytes % sizeof(int)) != 0)
    return fail(MC_EINVAL, "mc_config of %zu bytes: this library knows %zu (0.1 layout) .. %zu", cfg_bytes,
                offsetof(mc_config, fp8_linear), sizeof(mc_config));
  mc_config full;
  memset(&full, 0, sizeof(full));
  memcpy(&full, cfg, cfg_bytes);
  return mc_create(&full, out);
}

mc_status mc_create(const mc_config* cfg, mc_engine** out) {
  if (!cfg || !out) return fail(MC_EINVAL, "null argument");
  const mc_config& c = *cfg;
  if (c.dim <= 0 || c.num_heads <= 0 || c.dim != c.num_heads * 128)
    return fail(MC_EINVAL, "dim (%d) must be num_heads (%d) * 128", c.dim, c.num_heads);
  if ((c.dim % 256) || (c.ffn_dim % 64) || (c.text_dim % 64) || (c.freq_dim % 4) || c.num_layers <= 0)
    return fail(MC_EINVAL, "unsupported geometry dim=%d ffn=%d text_dim=%d", c.dim, c.ffn_dim, c.text_dim);
  if (c.sp_size < 1 || c.sp_rank < 0 || c.sp_rank >= c.sp_size) return fail(MC_EINVAL, "bad sp rank/size");
  MC_TRY(check_geometry(c.latent_f, c.latent_h, c.latent_w, c.sp_size));
  if (c.n_branches != 1 && c.n_branches != 2) return fail(MC_EINVAL, "n_branches must be 1 or 2");
  if (c.out_dim * 4 > 256) return fail(MC_EINVAL, "out_dim*4 > 256 unsupported by the head kernel");
  if (c.clip_dim < 0 || (c.clip_dim % 256) != 0) return fail(MC_EINVAL, "clip_dim %d must be 0 or a multiple of 256", c.clip_dim);
  if (c.vace_layers < 0 || (c.vace_layers > 0 && (c.vace_stride <= 0 || c.vace_in_dim <= 0 ||
                                                   (c.vace_layers - 1) * c.vace_stride >= c.num_layers)))
    return fail(MC_EINVAL, "bad VACE geometry: %d blocks, stride %d, in_dim %d", c.vace_layers, c.vace_stride, c.vace_in_dim);
  if ((c.no_context_cache | c.no_token_timesteps) & ~1) return fail(MC_EINVAL, "no_context_cache / no_token_timesteps must be 0 or 1");
  if (c.token_timestep_sets != 0 && (c.token_timestep_sets < 3 || c.token_timestep_sets > mc::kMaxTokenSets))
    return fail(MC_EINVAL, "token_timestep_sets must be 0 (two sets) or 3..%d, not %d", mc::kMaxTokenSets, c.token_timestep_sets);
  if (c.token_timestep_sets != 0 && c.no_token_timesteps)
    return fail(MC_EINVAL, "token_timestep_sets = %d with no_token_timesteps = 1", c.token_timestep_sets);
  if (c.fp8_linear < 0 || c.fp8_linear > 3)
    return fail(MC_EINVAL, "fp8_linear must be 0, 1 (per-row scales), 2 (MX block scales: QKV, FFN-1, FFN-2) or 3 (MX, the d x d Linears too)");
  if (c.fp8_linear && ((c.dim % 256) || (c.ffn_dim % 256) || c.dim < 512 || c.ffn_dim < 512))
    return fail(MC_EINVAL, "fp8_linear needs dim and ffn_dim to be multiples of 256 and >= 512");
  if (c.vace_layers > 0 && c.sp_size > 1 && (c.vace_layers - 1) * c.vace_stride == c.num_layers - 1)
    return fail(MC_EINVAL, "VACE with a hint on the last layer is single-GPU in this engine");

  std::unique_ptr<mc_engine, void (*)(mc_engine*)> own(new mc_engine(), mc_destroy);   // every early return frees it
  mc_engine* e = own.get();
  e->cfg = c;
  e->d = c.dim; e->ffn = c.ffn_dim; e->H = c.num_heads; e->NL = c.num_layers;
  e->P = c.sp_size; e->rank = c.sp_rank;
  e->sp = c.sp_size > 1 || c.sp_phases != 0;
  const Rows rows = derive_rows(c.latent_f, c.latent_h, c.latent_w, e->P, e->rank);
  e->L = rows.L; e->Lr = rows.Lr; e->Lp = rows.Lp; e->tok0 = rows.tok0;
  e->Kp = (int)align_up((size_t)c.in_dim * 4, 64);
  e->HT = (int)align_up((size_t)c.out_dim * 4, 64);
  e->ctx_rows = (int)align_up(c.text_len, 64);
  const size_t d = e->d, ffn = e->ffn;
  mc::WeightStore& W = e->weights;
  W.allow_f32_targets = true;   // adapters on the fp32 matrices below and deltas on the fp32 parameters (mc_lora_set / _set_delta)

  // fp8_linear only decides which Linears keep an e4m3 copy and of which kind: 1 = QKV, FFN-1, FFN-2 with per-row scales,
  // 2 = the same three with MX block scales, 3 = MX, the d x d Linears (self-attention O, cross-attention Q and O) too
  // options "mx_fp4" / "mx_fp6" (latched here): the element format of the MX copies.  dim and ffn_dim are multiples of 256 and
  // >= 512 by the fp8_linear check above, which is what the MX GEMMs ask of a Linear's k_in; checked again by name so that a
  // width the kernel cannot tile is refused here, never met at a launch
  MC_TRY(mc::latch_mx_format(c.fp8_linear >= 2, &e->mx_fmt));
  if (e->mx_fmt != mc::MX_E4M3) {
    MC_TRY(mc::check_mx_k(e->mx_fmt, "self_attn.q|k|v / ffn.0 / the dim x dim Linears (in_features = dim)", c.dim));
    MC_TRY(mc::check_mx_k(e->mx_fmt, "ffn.2 (in_features = ffn_dim)", c.ffn_dim));
  }
  const mc::MxFormat fmt = e->mx_fmt;
  const mc::Quant q_big = c.fp8_linear >= 2 ? mc::QUANT_MX : c.fp8_linear == 1 ? mc::QUANT_ROW : mc::QUANT_NONE;
  const mc::Quant q_dd = c.fp8_linear == 3 ? mc::QUANT_MX : mc::QUANT_NONE;
  e->layers.resize(e->NL);
  e->NV = c.vace_layers;
  e->vlayers.resize(e->NV);
  for (int i = 0; i < e->NL + e->NV; ++i) {
    const bool is_vace = i >= e->NL;
    Layer& l = is_vace ? e->vlayers[i - e->NL] : e->layers[i];
    l.index = i;
    const std::string p = (is_vace ? "vace_blocks." + std::to_string(i - e->NL) : "blocks." + std::to_string(i)) + ".";
    MC_TRY(W.add_linear(l.qkv, p + "self_attn.", {{"q", d}, {"k", d}, {"v", d}}, d, q_big, fmt));
    MC_TRY(W.add_linear(l.o, p + "self_attn.", {{"o", d}}, d, q_dd, fmt));
    MC_TRY(W.add_linear(l.cq, p + "cross_attn.", {{"q", d}}, d, q_dd, fmt));
    MC_TRY(W.add_linear(l.ckv, p + "cross_attn.", {{"k", d}, {"v", d}}, d));
    MC_TRY(W.add_linear(l.co, p + "cross_attn.", {{"o", d}}, d, q_dd, fmt));
    MC_TRY(W.add_linear(l.ffn1, p + "ffn.", {{"0", ffn}}, d, q_big, fmt));
    MC_TRY(W.add_linear(l.ffn2, p + "ffn.", {{"2", d}}, ffn, q_big, fmt));
    MC_TRY(W.add_f32(l.nq, p + "self_attn.norm_q.weight", d));
    MC_TRY(W.add_f32(l.nk, p + "self_attn.norm_k.weight", d));
    MC_TRY(W.add_f32(l.n3w, p + "norm3.weight", d));
    MC_TRY(W.add_f32(l.n3b, p + "norm3.bias", d));
    MC_TRY(W.add_f32(l.cnq, p + "cross_attn.norm_q.weight", d));
    MC_TRY(W.add_f32(l.cnk, p + "cross_attn.norm_k.weight", d));
    MC_TRY(W.add_f32(l.mod, p + "modulation", 6 * d));
    if (c.clip_dim > 0) {
      MC_TRY(W.add_linear(l.ckv_img, p + "cross_attn.", {{"k_img", d}, {"v_img", d}}, d));
      MC_TRY(W.add_f32(l.cnk_img, p + "cross_attn.norm_k_img.weight", d));
    }
  }
  if (e->NV > 0) {
    e->Kvp = (int)align_up((size_t)c.vace_in_dim * 4, 64);
    const size_t kv = (size_t)c.vace_in_dim * 4;
    if (kv != (size_t)e->Kvp) { return fail(MC_EINVAL, "vace_in_dim*4 must be a multiple of 64"); }
    MC_TRY(W.add_linear(e->vpatch, "", {{"vace_patch_embedding", d}}, kv));
    W.slots.at("vace_patch_embedding.weight").fixed = true;
    MC_TRY(W.add_linear(e->before, "vace_blocks.0.", {{"before_proj", d}}, d));
    MC_TRY(W.alloc(&e->vscale, d));
    e->after.resize(e->NV);
    for (int i = 0; i < e->NV; ++i)
      MC_TRY(W.add_linear(e->after[i], "vace_blocks." + std::to_string(i) + ".", {{"after_proj", d}}, d));
  }
  if (c.clip_dim > 0) {
    const size_t cd = c.clip_dim;
    e->img_rows = (int)align_up(257, 64);
    MC_TRY(W.add_f32(e->ln_img0_w, "img_emb.proj.0.weight", cd));
    MC_TRY(W.add_f32(e->ln_img0_b, "img_emb.proj.0.bias", cd));
    MC_TRY(W.add_linear(e->img1, "img_emb.proj.", {{"1", cd}}, cd));
    MC_TRY(W.add_linear(e->img3, "img_emb.proj.", {{"3", d}}, cd));
    MC_TRY(W.add_f32(e->ln_img4_w, "img_emb.proj.4.weight", d));
    MC_TRY(W.add_f32(e->ln_img4_b, "img_emb.proj.4.bias", d));
  }
  // patch weight [d, in_dim, 1, 2, 2] is stored [d, Kp] (Kp = in_dim*4 padded to a GEMM K step; the padding stays zero)
  const size_t kin = (size_t)c.in_dim * 4;
  MC_TRY(W.alloc_linear(e->patch, d, e->Kp));
  HIP_TRY(hipMemset(e->patch.w, 0, d * e->Kp * sizeof(bf16_t)));
  mc::Slot& w_patch = W.add_parts(e->patch, "", {{"patch_embedding", d}});
  w_patch.fixed = true;   // the patch embedders take no adapter, padded or not
  if (kin != (size_t)e->Kp) {
    w_patch.numel = d * kin;
    w_patch.pad = {d, kin, (size_t)e->Kp};
  }
  MC_TRY(W.add_linear(e->text0, "text_embedding.", {{"0", d}}, c.text_dim));
  MC_TRY(W.add_linear(e->text1, "text_embedding.", {{"2", d}}, d));
  MC_TRY(W.add_f32(e->w_time0, "time_embedding.0.weight", d * c.freq_dim, c.freq_dim));
  MC_TRY(W.add_f32(e->b_time0, "time_embedding.0.bias", d));
  MC_TRY(W.add_f32(e->w_time1, "time_embedding.2.weight", d * d, d));
  MC_TRY(W.add_f32(e->b_time1, "time_embedding.2.bias", d));
  MC_TRY(W.add_f32(e->w_tproj, "time_projection.1.weight", 6 * d * d, d));
  MC_TRY(W.add_f32(e->b_tproj, "time_projection.1.bias", 6 * d));
  MC_TRY(W.add_f32(e->w_head, "head.head.weight", (size_t)c.out_dim * 4 * d, d));
  MC_TRY(W.add_f32(e->b_head, "head.head.bias", (size_t)c.out_dim * 4));
  MC_TRY(W.add_f32(e->head_mod, "head.modulation", 2 * d));

  // RoPE table for this rank's rows: the two steps mc_set_geometry takes
  MC_TRY(rope_reserve(e, e->Lp, rope_axes_floats(c.latent_f, c.latent_h / 2, c.latent_w / 2)));
  MC_TRY(rope_build(e));

  // ---- workspace plan
  e->splitk_bytes = splitk_need(e, e->Lp);
  plan_workspace(e, rows, e->work);
  *out = own.release();
  return MC_OK;
}

void mc_destroy(mc_engine* e) {
  if (!e) return;
  e->weights.free_all();
  for (hipEvent_t ev : e->prof_ev) (void)hipEventDestroy(ev);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->side) (void)hipStreamDestroy(e->side);
  delete e;
}

size_t mc_workspace_bytes(const mc_engine* e) { return e ? e->work.need : 0; }

int mc_engine_token_timestep_sets(const mc_engine* e) {
  return !e || e->cfg.no_token_timesteps ? 0 : e->cfg.token_timestep_sets ? e->cfg.token_timestep_sets : 2;
}
int mc_engine_mx_fp4(const mc_engine* e) { return e && e->mx_fmt == mc::MX_E2M1 ? 1 : 0; }
int mc_engine_mx_fp6(const mc_engine* e) { return e && e->mx_fmt == mc::MX_E2M3 ? 1 : 0; }

mc_status mc_set_workspace(mc_engine* e, void* ws_dev, size_t bytes) {
  if (!e) return fail(MC_EINVAL, "null argument");
  MC_TRY(e->work.bind(ws_dev, bytes));
  return forget_workspace_state(e);
}

mc_status mc_geometry_bytes(const mc_engine* e, int latent_f, int latent_h, int latent_w, size_t* bytes) {
  if (!e || !bytes) return fail(MC_EINVAL, "null argument");
  MC_TRY(check_geometry(latent_f, latent_h, latent_w, e->P));
  mc::Workspace plan;
  plan_workspace(e, derive_rows(latent_f, latent_h, latent_w, e->P, e->rank), plan);
  *bytes = plan.need;
  return MC_OK;
}

mc_status mc_set_geometry(mc_engine* e, int latent_f, int latent_h, int latent_w) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->sp)
    return fail(MC_EINVAL, "mc_set_geometry: a sharded engine (sp_size %d%s) keeps the grid it was created with", e->P,
                e->cfg.sp_phases ? ", sp_phases" : "");
  if (e->phase_open) return fail(MC_ESTATE, "mc_set_geometry between mc_embed and mc_head");
  MC_TRY(check_geometry(latent_f, latent_h, latent_w, e->P));
  const Rows r = derive_rows(latent_f, latent_h, latent_w, e->P, e->rank);
  mc::Workspace plan;
  plan_workspace(e, r, plan);
  if (e->work.ws && plan.need > e->work.bound)
    return fail(MC_EINVAL, "latent grid %dx%dx%d needs a workspace of %zu bytes, %zu bytes are bound (mc_set_workspace)", latent_f,
                latent_h, latent_w, plan.need, e->work.bound);
  // earlier forwards may still be reading the RoPE table and the buffers of the old plan
  HIP_TRY(hipDeviceSynchronize());
  // the one step that can fail for lack of memory: before anything changes
  MC_TRY(rope_reserve(e, r.Lp, rope_axes_floats(latent_f, latent_h / 2, latent_w / 2)));
  MC_TRY(e->work.replan(plan));
  e->cfg.latent_f = latent_f; e->cfg.latent_h = latent_h; e->cfg.latent_w = latent_w;
  e->L = r.L; e->Lr = r.Lr; e->Lp = r.Lp; e->tok0 = r.tok0;
  MC_TRY(rope_build(e));
  return forget_workspace_state(e);
}

mc_status mc_buffer_info(const mc_engine* e, const char* name, size_t* offset, size_t* bytes) {
  if (!e || !name) return fail(MC_EINVAL, "null argument");
  std::string n(name);
  if (n == "residual_branch0" || n == "residual_branch1") {  // the slot currently held by a branch
    static const char* names[3] = {"residual0", "residual1", "residual2"};
    n = names[e->res_slot[n.back() - '0']];
  }
  return e->work.info(n, offset, bytes);
}

mc_status mc_set_weight(mc_engine* e, const char* name, const void* src_dev, mc_dtype dtype, const int64_t* shape,
                        int ndim, mc_stream stream) {
  if (e) {  // any cached text context was computed with the old weights
    e->ctx_valid[0] = e->ctx_valid[1] = false;
    e->ctx_active = -1;
    e->pair_drop();   // and so was a kept front
  }
  if (!e || !name || !src_dev || !shape) return fail(MC_EINVAL, "null argument");
  return e->weights.set(name, src_dev, dtype, shape, ndim, (hipStream_t)stream);
}

int mc_weights_missing(const mc_engine* e, char* buf, size_t buflen) { return e ? e->weights.missing(buf, buflen) : -1; }

// ---- LoRA adapters: the store does the work (host.h), between forwards only
static mc_status lora_entry(const mc_engine* e, const char* what) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->pair != mc_engine::PAIR_NONE) return fail(MC_ESTATE, "%s between mc_pair_begin and mc_pair_end", what);
  if (e->phase_open) return fail(MC_ESTATE, "%s between mc_embed and mc_head", what);
  return MC_OK;
}

mc_status mc_lora_set(mc_engine* e, const char* adapter, const char* weight_name, const void* down_dev, const int64_t* down_shape,
                      const void* up_dev, const int64_t* up_shape, mc_dtype dtype, float factor, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_lora_set"));
  return e->weights.lora_set(adapter, weight_name, down_dev, down_shape, up_dev, up_shape, dtype, factor, (hipStream_t)stream);
}

mc_status mc_lora_set_delta(mc_engine* e, const char* adapter, const char* param_name, const void* delta_dev, size_t numel,
                            mc_dtype dtype, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_lora_set_delta"));
  return e->weights.lora_set_delta(adapter, param_name, delta_dev, numel, dtype, (hipStream_t)stream);
}

mc_status mc_lora_set_kron(mc_engine* e, const char* adapter, const char* weight_name, const void* w1_dev, const int64_t* w1_shape,
                           const void* w2_dev, const int64_t* w2_shape, mc_dtype dtype, float factor, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_lora_set_kron"));
  return e->weights.lora_set_kron(adapter, weight_name, w1_dev, w1_shape, w2_dev, w2_shape, dtype, factor, (hipStream_t)stream);
}

mc_status mc_lora_set_hada(mc_engine* e, const char* adapter, const char* weight_name, const void* u1_dev, const int64_t* u_shape,
                           const void* d1_dev, const int64_t* d_shape, const void* u2_dev, const void* d2_dev, mc_dtype dtype,
                           float factor, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_lora_set_hada"));
  return e->weights.lora_set_hada(adapter, weight_name, u1_dev, u_shape, d1_dev, d_shape, u2_dev, d2_dev, dtype, factor,
                                  (hipStream_t)stream);
}

mc_status mc_lora_set_magnitude(mc_engine* e, const char* adapter, const char* weight_name, const void* magnitude_dev, size_t numel,
                                mc_dtype dtype, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_lora_set_magnitude"));
  return e->weights.lora_set_magnitude(adapter, weight_name, magnitude_dev, numel, dtype, (hipStream_t)stream);
}

mc_status mc_lora_scale(mc_engine* e, const char* adapter, float scale) {
  MC_TRY(lora_entry(e, "mc_lora_scale"));
  return e->weights.lora_scale(adapter, scale);
}

mc_status mc_lora_remove(mc_engine* e, const char* adapter) {
  MC_TRY(lora_entry(e, "mc_lora_remove"));
  return e->weights.lora_remove(adapter);
}

// Everything the engine derived from weights goes with a merge, as with mc_set_weight, and the two contexts that call keeps
// as well: the cached text contexts, the CLIP context, the VACE c0 and a kept pair front.  The MagCache state stays.
mc_status mc_lora_apply(mc_engine* e, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_lora_apply"));
  int merged = 0;
  const mc_status st = e->weights.lora_apply((hipStream_t)stream, &merged);
  if (merged > 0) {
    e->ctx_valid[0] = e->ctx_valid[1] = false;
    e->ctx_active = -1;
    e->have_clip = e->have_vace = false;
    e->pair_drop();
  }
  return st;
}

mc_status mc_lora_info(const mc_engine* e, int* adapters, int* params, size_t* base_bytes) {
  if (!e) return fail(MC_EINVAL, "null engine");
  e->weights.lora_info(adapters, params, base_bytes);
  return MC_OK;
}

// I2V: context_clip = img_emb(clip_fea)   (reference :264-266; upstream MLPProj: LayerNorm, Linear, GELU(erf),
// Linear, LayerNorm).  257 tokens; rows up to img_rows are padding (finite, masked in the attention).
mc_status mc_set_clip_fea(mc_engine* e, const void* clip_dev, mc_dtype dtype, int n_tokens, mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  MC_TRY(check_ready(e));
  e->pair_drop();
  const mc_config& c = e->cfg;
  if (c.clip_dim <= 0) return fail(MC_EINVAL, "engine was created without clip_dim (t2v model)");
  if (!clip_dev || n_tokens != 257) return fail(MC_EINVAL, "clip_fea must be [257, %d]", c.clip_dim);
  const int cd = c.clip_dim, ir = e->img_rows, d = e->d;
  float* in = e->buf<float>("clip_in");
  HIP_TRY(hipMemsetAsync(in, 0, (size_t)ir * cd * 4, s));
  if (dtype == MC_F32) {
    HIP_TRY(hipMemcpyAsync(in, clip_dev, (size_t)n_tokens * cd * 4, hipMemcpyDeviceToDevice, s));
  } else {
    return fail(MC_EINVAL, "clip_fea must be given as fp32");
  }
  bf16_t* n0 = e->buf<bf16_t>("clip_n");
  HIP_TRY(mc::launch_ln_modulate(in, cd, nullptr, 0, e->ln_img0_w, e->ln_img0_b, 1, 1e-5f, n0, cd, nullptr, 0, ir, cd, s));
  MC_TRY(linear_bf16_out(e, e->img1, ir, ActSrc{n0, cd}, e->buf<bf16_t>("clip_h"), mc::EPI_GELU_ERF_BF16, s));
  // autocast: the Linear's output is bf16 before the LayerNorm
  MC_TRY(linear_bf16_out(e, e->img3, ir, ActSrc{e->buf<bf16_t>("clip_h"), cd}, e->buf<bf16_t>("clip_h2"), mc::EPI_BF16, s));
  // LayerNorm of the bf16 rows: the kernel's (fp32 x) + (bf16 x0) form with x = 0
  HIP_TRY(hipMemsetAsync(e->buf<float>("clip_o"), 0, (size_t)ir * d * 4, s));
  HIP_TRY(mc::launch_ln_modulate(e->buf<float>("clip_o"), d, e->buf<bf16_t>("clip_h2"), d, e->ln_img4_w,
                                 e->ln_img4_b, 1, 1e-5f, e->buf<bf16_t>("ctx_img"), d, nullptr, 0, ir, d, s));
  e->have_clip = true;
  return MC_OK;
}

// VACE: c0 = vace_patch_embedding(vace_context) (upstream forward_vace; reference call site :544), constant over a
// video, and the hint scale (vace_context_scale, :546).
mc_status mc_set_vace_context(mc_engine* e, const float* vace_dev, float context_scale, mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  MC_TRY(check_ready(e));
  e->pair_drop();
  if (e->NV <= 0) return fail(MC_EINVAL, "engine was created without VACE blocks");
  const mc_config& c = e->cfg;
  const int d = e->d;
  if (vace_dev) {
    bf16_t* vt = e->buf<bf16_t>("vtokens");
    HIP_TRY(mc::launch_patchify(vace_dev, c.vace_in_dim, c.latent_f, c.latent_h, c.latent_w, e->tok0, e->Lr, e->Lp, vt,
                                e->Kvp, s));
    mc::GemmParams p = {};
    p.X = e->buf<float>("xc"); p.ldx = d;
    p.X0out = e->buf<bf16_t>("c0"); p.ldx0out = d;
    p.m_valid = e->Lr;
    MC_TRY(linear(e, e->vpatch, whole(e->vpatch), e->Lp, ActSrc{vt, e->Kvp}, p, mc::EPI_EMBED, s));
    e->have_vace = true;
  } else if (!e->have_vace) {
    return fail(MC_EINVAL, "null vace_context and none set before");
  }
  std::vector<float> sc(d, context_scale);
  HIP_TRY(hipMemcpyAsync(e->vscale, sc.data(), (size_t)d * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));   // sc is a host temporary
  return MC_OK;
}

// ------------------------------------------------------------------------------------------------
// embeds: patch embedding, time embedding + projection, text embedding   (reference :236-262)
// context = text_embedding(zero-padded context) -> dst [ctx_rows, d] bf16   (:256-262)
static mc_status embed_context(mc_engine* e, const void* context_dev, mc_dtype ctx_dtype, int ctx_len, bf16_t* dst,
                               hipStream_t s) {
  const mc_config& c = e->cfg;
  if (ctx_len <= 0 || ctx_len > c.text_len)
    return fail(MC_EINVAL, "context length %d exceeds text_len %d", ctx_len, c.text_len);
  bf16_t* ctx_in = e->buf<bf16_t>("ctx_in");
  if (ctx_dtype == MC_F32) {
    HIP_TRY(mc::launch_cast_pad_bf16((const float*)context_dev, c.text_dim, ctx_len, e->ctx_rows, c.text_dim, ctx_in,
                                     c.text_dim, s));
  } else {
    HIP_TRY(hipMemsetAsync(ctx_in, 0, (size_t)e->ctx_rows * c.text_dim * 2, s));
    HIP_TRY(hipMemcpyAsync(ctx_in, context_dev, (size_t)ctx_len * c.text_dim * 2, hipMemcpyDeviceToDevice, s));
  }
  bf16_t* ctx_h = e->buf<bf16_t>("ctx_h");
  MC_TRY(linear_bf16_out(e, e->text0, e->ctx_rows, ActSrc{ctx_in, c.text_dim}, ctx_h, mc::EPI_GELU_BF16, s));
  return linear_bf16_out(e, e->text1, e->ctx_rows, ActSrc{ctx_h, e->d}, dst, mc::EPI_BF16, s);
}

// the cross-attention K|V of one block for a context: k = norm_k(k(ctx)), v = v(ctx)  (upstream WanT2VCrossAttention)
static mc_status context_kv(mc_engine* e, const Layer& l, const bf16_t* ctx, bf16_t* ckv, hipStream_t s) {
  const int d = e->d;
  MC_TRY(linear_bf16_out(e, l.ckv, e->ctx_rows, ActSrc{ctx, d}, ckv, mc::EPI_BF16, s));
  HIP_TRY(mc::launch_rmsnorm_rope(ckv, 2 * d, l.cnk, e->cfg.eps, nullptr, 0, e->ctx_rows, d, s));
  return MC_OK;
}

// The embeds that depend on the latent and on t -- patch embedding -> x (fp32: "x", or "pair_x" for the first forward of a
// CFG pair) and ori_x ("x0"), the time embedding, every modulation vector -- and nothing that depends on the context: what
// the second forward of a CFG pair reuses.
static mc_status embed_latent_time(mc_engine* e, const float* latent_dev, const float* t_dev, double t_host, float* x,
                                   hipStream_t s) {
  const mc_config& c = e->cfg;
  const int d = e->d;
  // x = patch_embedding(latent): im2col -> GEMM, x (fp32) and ori_x (bf16), zero rows past seq_len
  bf16_t* tokens = e->buf<bf16_t>("tokens");
  if (e->Kp != c.in_dim * 4) HIP_TRY(hipMemsetAsync(tokens, 0, (size_t)e->Lp * e->Kp * 2, s));
  HIP_TRY(mc::launch_patchify(latent_dev, c.in_dim, c.latent_f, c.latent_h, c.latent_w, e->tok0, e->Lr, e->Lp,
                              tokens, e->Kp, s));
  {
    mc::GemmParams p = {};
    p.X = x; p.ldx = d;
    p.X0out = e->buf<bf16_t>("x0"); p.ldx0out = d;
    p.m_valid = e->Lr;
    MC_TRY(linear(e, e->patch, whole(e->patch), e->Lp, ActSrc{tokens, e->Kp}, p, mc::EPI_EMBED, s));
  }
  // e = time_embedding(sinusoidal(t)) ; e0 = time_projection(e)   (fp32, :249-253).  With per-token timesteps
  // (Wan2.2, MagCache4Wan2.2/magcache_generate.py:261-270: e [B, seq_len, d], e0 [B, seq_len, 6, d]) the same chain
  // runs for the two values the tokens carry -- max (set 0) and min (set 1) -- and every consumer selects per token.
  const int n_sets = e->tok_t ? 2 : 1;
  float* t2 = e->buf<float>("tok_t2");
  const size_t temb_set = (size_t)c.freq_dim + 2 * d + 6 * d, emod_set = (size_t)(e->NL + e->NV) * 6 * d;
  if (e->tok_t && c.token_timestep_sets) {
    // a capacity engine: the distinct values in one pass ("tok_vals", descending, padded), then the SAME chain over all C
    // sets at once -- seven launches whatever C is, every weight row read once, every set's bits those of the loop below
    const int C = c.token_timestep_sets;
    float* vals = e->buf<float>("tok_vals");
    HIP_TRY(mc::launch_token_t_sets(e->tok_t, e->L, e->tok0, e->Lr, e->Lp, C, t2, vals, e->buf<uint8_t>("tok_sel"), s));
    float* temb = e->buf<float>("temb");
    float* h1 = temb + c.freq_dim;
    float* ev = h1 + d;
    float* e0 = ev + d;
    const long ts = (long)temb_set;
    HIP_TRY(mc::launch_sinusoid_rows(vals, C, c.freq_dim, temb, ts, s));
    HIP_TRY(mc::launch_gemv_f32_rows(e->w_time0, temb, ts, e->b_time0, h1, ts, C, d, c.freq_dim, 0, 1, s));
    HIP_TRY(mc::launch_gemv_f32_rows(e->w_time1, h1, ts, e->b_time1, ev, ts, C, d, d, 0, 0, s));
    HIP_TRY(mc::launch_gemv_f32_rows(e->w_tproj, ev, ts, e->b_tproj, e0, ts, C, 6 * d, d, 1, 0, s));
    std::vector<const float*> mods(e->NL + e->NV);
    for (int l = 0; l < e->NL + e->NV; ++l) mods[l] = e->layer(l).mod;
    HIP_TRY(mc::launch_add_bcast_rows(e0, ts, C, 6 * d, mods.data(), (int)mods.size(), 6 * d, e->buf<float>("emod"), (long)emod_set, s));
    const float* hm = e->head_mod;
    HIP_TRY(mc::launch_add_bcast_rows(ev, ts, C, d, &hm, 1, 2 * d, e->buf<float>("ehead"), 2 * d, s));
    return MC_OK;
  }
  if (e->tok_t)
    HIP_TRY(mc::launch_token_t_prepare(e->tok_t, e->L, e->tok0, e->Lr, e->Lp, t2, e->buf<uint8_t>("tok_sel"), s));
  for (int set = 0; set < n_sets; ++set) {
    float* temb = e->buf<float>("temb") + set * temb_set;
    float* sinus = temb;
    float* h1 = temb + c.freq_dim;
    float* ev = h1 + d;
    float* e0 = ev + d;
    HIP_TRY(mc::launch_sinusoid(e->tok_t ? t2 + set : t_dev, t_host, c.freq_dim, sinus, s));
    HIP_TRY(mc::launch_gemv_f32(e->w_time0, sinus, e->b_time0, h1, d, c.freq_dim, 0, 1, s));
    HIP_TRY(mc::launch_gemv_f32(e->w_time1, h1, e->b_time1, ev, d, d, 0, 0, s));
    HIP_TRY(mc::launch_gemv_f32(e->w_tproj, ev, e->b_tproj, e0, 6 * d, d, 1, 0, s));
    // per-layer modulation vectors (block.modulation + e0) and the head's (head.modulation + e)
    float* emod = e->buf<float>("emod") + set * emod_set;
    for (int l = 0; l < e->NL + e->NV; ++l)
      HIP_TRY(mc::launch_add_bcast(e0, 6 * d, e->layer(l).mod, emod + (size_t)l * 6 * d, 6 * d, s));
    HIP_TRY(mc::launch_add_bcast(ev, d, e->head_mod, e->buf<float>("ehead") + set * 2 * d, 2 * d, s));
  }
  return MC_OK;
}

// context = text_embedding(zero-padded context)   (:256-262); NULL: the slot selected by mc_set_context / mc_use_context
static mc_status embed_text(mc_engine* e, const void* context_dev, mc_dtype ctx_dtype, int ctx_len, hipStream_t s) {
  if (context_dev) {
    e->ctx_active = -1;
    return embed_context(e, context_dev, ctx_dtype, ctx_len, e->buf<bf16_t>("ctx"), s);
  }
  if (e->ctx_active < 0 || !e->ctx_valid[e->ctx_active])
    return fail(MC_ESTATE, "context_dev is NULL but no cached context is selected (mc_set_context)");
  return MC_OK;
}

static mc_status embed(mc_engine* e, const float* latent_dev, const float* t_dev, double t_host, const void* context_dev,
                       mc_dtype ctx_dtype, int ctx_len, float* x, hipStream_t s) {
  MC_TRY(check_ready(e));
  if (!latent_dev) return fail(MC_EINVAL, "null input");
  if (e->cfg.clip_dim > 0 && !e->have_clip)
    return fail(MC_ESTATE, "i2v model: mc_set_clip_fea must run before the forward (reference assert :226-227)");
  Prof pr(e, MC_PROF_EMBED, s);
  MC_TRY(embed_latent_time(e, latent_dev, t_dev, t_host, x, s));
  MC_TRY(embed_text(e, context_dev, ctx_dtype, ctx_len, s));
  e->embedded = true;
  return MC_OK;
}

mc_status mc_embed(mc_engine* e, const float* latent_dev, const float* t_dev, double t_host,
                   const void* context_dev, mc_dtype ctx_dtype, int ctx_len, mc_stream stream_) {
  if (e) e->pair_drop();   // a phase call rewrites the embeds a kept front consists of
  const mc_status st = embed(e, latent_dev, t_dev, t_host, context_dev, ctx_dtype, ctx_len, e ? e->buf<float>("x") : nullptr,
                             (hipStream_t)stream_);
  if (e && st == MC_OK) e->phase_open = true;   // until mc_head: the grid stays (mc_set_geometry)
  return st;
}

// LayerNorm + modulate of x for the Linear `l`, as that Linear's activation source: with fp8_fused_quant an fp8 Linear's row
// goes straight to "aq" (+ scales); otherwise the bf16 row goes to "xn" as ever (and an fp8 Linear quantises it).
// set_stride != 0: sc / sh are the first of the engine's token_timestep_sets sets, set_stride floats apart (sc2 / sh2 unused)
static mc_status ln_for_gemm(mc_engine* e, const Linear& l, const float* x, const float* sc, const float* sh, int mode,
                             const float* sc2, const float* sh2, const uint8_t* sel, hipStream_t s, ActSrc* a,
                             long set_stride = 0) {
  const int n_sets = set_stride ? e->cfg.token_timestep_sets : 0;
  const int d = e->d, Lp = e->Lp;
  bf16_t* xn = e->buf<bf16_t>("xn");
  *a = ActSrc{xn, d, fused_quant(l)};
  if (a->quantised) {
    HIP_TRY(mc::launch_ln_modulate_fp8(x, d, sc, sh, mode, e->cfg.eps, e->buf<uint8_t>("aq"), d,
                                       l.mx ? nullptr : e->buf<float>("a_scale"), l.mx ? e->buf<uint8_t>("a_mx") : nullptr,
                                       (long)Lp, Lp, d, s, sc2, sh2, sel, set_stride, n_sets));
  } else {
    HIP_TRY(mc::launch_ln_modulate(x, d, nullptr, 0, sc, sh, mode, e->cfg.eps, xn, d, nullptr, 0, Lp, d, s, sc2, sh2, sel,
                                   set_stride, n_sets));
  }
  return MC_OK;
}

// l / em / x: the block's weights, its 6 modulation vectors and the residual stream it works on (the main stream
// "x", or the VACE control stream "xc")
// em2 / sel: the second modulation set (em + one "emod" set) and the per-token selector when per-token timesteps are on
// A capacity engine (token_timestep_sets) has no "second" set: its consumers get (em, set_stride, sel) and take row
// min(sel, C - 1) of the table of sets that starts at em.
static const float* second_set(const mc_engine* e, const float* em) {
  return e->tok_t && !e->cfg.token_timestep_sets ? em + (size_t)(e->NL + e->NV) * 6 * e->d : nullptr;
}
static long set_stride(const mc_engine* e) {
  return e->tok_t && e->cfg.token_timestep_sets ? (long)(e->NL + e->NV) * 6 * e->d : 0;
}
static void gate_table(const mc_engine* e, mc::GemmParams& p) {
  if (const long st = set_stride(e)) { p.gate_sel = e->buf<uint8_t>("tok_sel"); p.gate_stride = st; p.gate_sets = e->cfg.token_timestep_sets; }
}
static const uint8_t* tok_sel(const mc_engine* e) { return e->tok_t ? e->buf<uint8_t>("tok_sel") : nullptr; }

// LayerNorm + modulate -> "xn"; one device: q|k|v Linear -> "qkv", RMSNorm + RoPE of q and k (everything before attention).
// Sequence parallel: only what the OTHER ranks wait for -- the [k|v] Linear into "kv_local" and the k norm / RoPE --, so that
// the caller can start the all-gather before this rank's q exists (block_pre_q).
static mc_status block_pre_kv(mc_engine* e, const Layer& l, const float* em, float* x, hipStream_t s) {
  const int d = e->d, Lp = e->Lp;
  const float* em2 = second_set(e, em);
  ActSrc a;
  {
    Prof pr(e, MC_PROF_LN_MODULATE, s);
    MC_TRY(ln_for_gemm(e, l.qkv, x, em + d, em, 0, em2 ? em2 + d : nullptr, em2, tok_sel(e), s, &a, set_stride(e)));
  }
  mc::GemmParams p = {};
  if (!e->sp) {
    bf16_t* qkv = e->buf<bf16_t>("qkv");
    p.Cb = qkv; p.ldc = 3 * d;
    {
      Prof pr(e, MC_PROF_GEMM_QKV, s);
      MC_TRY(linear(e, l.qkv, whole(l.qkv), Lp, a, p, mc::EPI_BF16, s));
    }
    Prof pr(e, MC_PROF_RMSNORM_ROPE, s);
    HIP_TRY(mc::launch_rmsnorm_rope(qkv, 3 * d, l.nq, e->cfg.eps, e->cs_table, 0, Lp, d, s));
    HIP_TRY(mc::launch_rmsnorm_rope(qkv + d, 3 * d, l.nk, e->cfg.eps, e->cs_table, 0, Lp, d, s));
  } else {
    // [k|v] -> "kv_local" (ld 2d): the rows every other rank needs, first.  An fp8 Linear quantises the activation rows once
    // ("aq": the fused LayerNorm, or this launch) and block_pre_q reuses them
    bf16_t* kvl = e->buf<bf16_t>("kv_local");
    p.Cb = kvl; p.ldc = 2 * d;
    {
      Prof pr(e, MC_PROF_GEMM_QKV, s);
      MC_TRY(linear(e, l.qkv, RowRange{d, 2 * d}, Lp, a, p, mc::EPI_BF16, s));
    }
    Prof pr(e, MC_PROF_RMSNORM_ROPE, s);
    HIP_TRY(mc::launch_rmsnorm_rope(kvl, 2 * d, l.nk, e->cfg.eps, e->cs_table, 0, Lp, d, s));
  }
  e->attn_layer = -2;   // a new layer: no attention chain open
  return MC_OK;
}

// sequence parallel only: q Linear of the rows block_pre_kv normalised ("xn", or quantised in "aq") -> "qkv"[:, :d] (ld d),
// q norm / RoPE; runs beside the all-gather the caller started in between
static mc_status block_pre_q(mc_engine* e, const Layer& l, hipStream_t s) {
  const int d = e->d, Lp = e->Lp;
  if (!e->sp) return MC_OK;
  bf16_t* qkv = e->buf<bf16_t>("qkv");
  {
    Prof pr(e, MC_PROF_GEMM_QKV, s);
    mc::GemmParams p = {};
    p.Cb = qkv; p.ldc = d;
    MC_TRY(linear(e, l.qkv, RowRange{0, d}, Lp, ActSrc{e->buf<bf16_t>("xn"), d, true}, p, mc::EPI_BF16, s));
  }
  Prof pr(e, MC_PROF_RMSNORM_ROPE, s);
  HIP_TRY(mc::launch_rmsnorm_rope(qkv, d, l.nq, e->cfg.eps, e->cs_table, 0, Lp, d, s));
  return MC_OK;
}

static mc_status block_pre(mc_engine* e, const Layer& l, const float* em, float* x, hipStream_t s) {
  MC_TRY(block_pre_kv(e, l, em, x, s));
  return block_pre_q(e, l, s);
}

static mc_status check_layer_call(mc_engine* e, int layer) {
  if (!e || !e->embedded) return fail(MC_ESTATE, "mc_embed must run first");
  if (layer < 0 || layer >= e->NL) return fail(MC_EINVAL, "layer %d out of range", layer);
  return MC_OK;
}

mc_status mc_block_pre_attn(mc_engine* e, int layer, mc_stream stream_) {
  MC_TRY(check_layer_call(e, layer));
  e->pair_drop();   // a phase call works on "x", where a kept front lies
  return block_pre(e, e->layers[layer], e->emod(e->layers[layer]), e->buf<float>("x"), (hipStream_t)stream_);
}

// The two halves of mc_block_pre_attn (sp_size > 1): a caller that starts its all-gather between them overlaps it with the q
// Linear as well.  mc_block_pre_attn == mc_block_pre_kv + mc_block_pre_q.
mc_status mc_block_pre_kv(mc_engine* e, int layer, mc_stream stream_) {
  MC_TRY(check_layer_call(e, layer));
  if (!e->sp) return fail(MC_ESTATE, "mc_block_pre_kv needs a sequence-parallel engine (sp_size > 1 or sp_phases) (one GPU: mc_block_pre_attn / mc_forward)");
  e->pair_drop();
  return block_pre_kv(e, e->layers[layer], e->emod(e->layers[layer]), e->buf<float>("x"), (hipStream_t)stream_);
}

mc_status mc_block_pre_q(mc_engine* e, int layer, mc_stream stream_) {
  MC_TRY(check_layer_call(e, layer));
  if (!e->sp) return fail(MC_ESTATE, "mc_block_pre_q needs a sequence-parallel engine (sp_size > 1 or sp_phases)");
  e->pair_drop();
  return block_pre_q(e, e->layers[layer], (hipStream_t)stream_);
}

// One launch of a layer's self-attention chain (sp_size > 1).  round < 0: this rank's own shard ("kv_local", needs nothing
// from the other ranks); round c >= 0: chunk c of the gathered shards ("kv_gather"[c] = [P][Lp / C][2d]), without this
// rank's shard when the local launch already covered it.  The first launch of a chain writes "ao" and the log2-sum-exp of
// the keys it visited ("attn_lse"); every later one merges into both in the kernel epilogue (in place).
static mc_status sp_attn_launch(mc_engine* e, int layer, int round, hipStream_t s) {
  attn_chain_open(e, layer);
  const int n_rounds = sp_rounds(e);
  bool more;   // does another launch of this chain follow?
  if (round < 0) {
    if (e->attn_launches) return fail(MC_ESTATE, "the local-shard attention must be the first launch of a layer's chain");
    more = true;
  } else {
    if (round != e->attn_rounds_done || round >= n_rounds)
      return fail(MC_ESTATE, "attention round %d out of order (rounds done %d of %d)", round, e->attn_rounds_done, n_rounds);
    more = round + 1 < n_rounds;
    if (e->attn_local_done && e->P == 1) {   // a world of one (sp_phases): the local launch covered every key
      e->attn_rounds_done++;
      return MC_OK;
    }
  }
  float* lse = e->buf<float>("attn_lse");
  {
    Prof pr(e, MC_PROF_ATTN_SELF, s);   // measurement hook, see mc_profile_enable
    MC_TRY(attend(e, e->buf<bf16_t>("qkv"), e->d, e->buf<bf16_t>("ao"), sp_keys(e, round, e->attn_local_done),
                  e->attn_launches ? lse : nullptr, more ? lse : nullptr, s));
  }
  e->attn_launches++;
  if (round < 0) e->attn_local_done = true; else e->attn_rounds_done++;
  return MC_OK;
}

// One launch of the chain as an INDEPENDENT partial result: slot 0 = this rank's own shard, slot 1 + c = gather round c
// without this rank's shard; normalised O -> "ao_part"[slot], log2-sum-exp -> "lse_part"[slot]; nothing is merged here.
static mc_status sp_attn_partial(mc_engine* e, int round, hipStream_t s) {   // (timed by the caller: one pair around the chain)
  const size_t slot = round < 0 ? 0 : 1 + round;
  return attend(e, e->buf<bf16_t>("qkv"), e->d, e->buf<bf16_t>("ao_part") + slot * e->Lp * e->d, sp_keys(e, round, true), nullptr,
                e->buf<float>("lse_part") + slot * e->H * e->Lp, s);
}

static mc_status sp_side_stream(mc_engine* e) {
  if (e->side) return MC_OK;
  HIP_TRY(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
  return MC_OK;
}

// Self-attention over this rank's own K/V shard ("kv_local"): normalised partial result -> "ao", log2-sum-exp ->
// "attn_lse".  Needs nothing from the other ranks, so the caller overlaps it with the all-gather.
mc_status mc_block_attn_local(mc_engine* e, int layer, mc_stream stream_) {
  MC_TRY(check_layer_call(e, layer));
  if (!e->sp) return fail(MC_ESTATE, "mc_block_attn_local needs a sequence-parallel engine (sp_size > 1 or sp_phases)");
  return sp_attn_launch(e, layer, -1, (hipStream_t)stream_);
}

// Self-attention over round `round` of the gathered shards (rounds in order 0 .. mc_sp_rounds - 1; the caller has made
// `stream` wait for that round of its all-gather).  mc_block_post_attn attends whatever rounds are still missing.
mc_status mc_block_attn_round(mc_engine* e, int layer, int round, mc_stream stream_) {
  MC_TRY(check_layer_call(e, layer));
  if (!e->sp) return fail(MC_ESTATE, "mc_block_attn_round needs a sequence-parallel engine (sp_size > 1 or sp_phases)");
  if (round < 0) return fail(MC_EINVAL, "round %d", round);
  return sp_attn_launch(e, layer, round, (hipStream_t)stream_);
}

// Rounds of the K|V all-gather per layer: round c moves rows [c Lp / C, (c + 1) Lp / C) of every rank's "kv_local" into
// "kv_gather"[c] ([P][Lp / C][2 dim] bf16), and the attention over it runs while round c + 1 is on the wire.  C = 1 is one
// all-gather of whole shards.  Lp / C must be a multiple of 64 (Lp is a multiple of 256: 1, 2 and 4 always work).
mc_status mc_sp_set_chunks(mc_engine* e, int chunks) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (!e->sp) return fail(MC_ESTATE, "mc_sp_set_chunks needs a sequence-parallel engine (sp_size > 1 or sp_phases)");
  if (chunks < 1 || chunks > 64 || e->Lp % chunks || (e->Lp / chunks) % 64)
    return fail(MC_EINVAL, "sp chunks %d: rows per shard %d / chunks must be a multiple of 64", chunks, e->Lp);
  e->sp_chunks = chunks;
  e->attn_layer = -2;
  e->pair_drop();
  return MC_OK;
}

mc_status mc_sp_geometry(const mc_engine* e, int* num_layers, int* seq_len, int* rows_per_rank, int* head_stride, int* dim,
                         int* sp_size) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (num_layers) *num_layers = e->NL;
  if (seq_len) *seq_len = e->L;
  if (rows_per_rank) *rows_per_rank = e->Lr;
  if (head_stride) *head_stride = e->HT;
  if (dim) *dim = e->d;
  if (sp_size) *sp_size = e->P;
  return MC_OK;
}

void* mc_workspace_base(const mc_engine* e) { return e ? (void*)e->work.ws : nullptr; }

// geometry of round `round` (NULL outputs are skipped): rows per shard chunk, valid keys at the start of each, and the
// number of rounds that carry valid keys (later rounds hold padding only: neither gathered nor attended)
mc_status mc_sp_round_info(const mc_engine* e, int round, int* n_rounds, int* chunk_rows, int* valid) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (round < 0 || round >= e->sp_chunks) return fail(MC_EINVAL, "round %d of %d", round, e->sp_chunks);
  if (n_rounds) *n_rounds = e->sp ? sp_rounds(e) : 0;
  if (chunk_rows) *chunk_rows = sp_chunk_rows(e);
  if (valid) *valid = sp_round_valid(e, round);
  return MC_OK;
}

// attention -> o (+gated residual) -> norm3 -> cross-attn (+residual) -> LN+mod -> FFN (+gated residual), in two halves that
// meet where the text context enters the block:
//   block_post_self  self-attention, o (+gated residual), norm3, the cross-attention q Linear and its RMSNorm -> cq
//   block_post_ctx   cross-attention over the context's K|V (+residual), LN+mod, FFN (+gated residual)
// layer: main-layer index (sequence-parallel two-phase bookkeeping), -1 for a VACE block.  capture: fuse the MagCache
// residual capture into the last epilogue (the last main layer, unless a VACE hint is still to be added to it).
// cq [Lp][d]: the normalised cross-attention q rows -- the head of "qkv" (the self-attention q/k/v are dead by then), or
// "pair_cq" in the two forwards of a CFG pair.
static mc_status block_post_self(mc_engine* e, const Layer& l, const float* em, float* x, int layer, bf16_t* cq, hipStream_t s) {
  const int d = e->d, Lp = e->Lp;
  bf16_t* ao = e->buf<bf16_t>("ao");
  const float* em2 = second_set(e, em);
  const uint8_t* sel = tok_sel(e);

  // ---- self attention over the full sequence
  if (!e->sp) {
    Prof pr(e, MC_PROF_ATTN_SELF, s);
    MC_TRY(attend(e, e->buf<bf16_t>("qkv"), 3 * d, ao, qkv_keys(e), nullptr, nullptr, s));
  } else {
    // whatever the caller has not attended yet (mc_block_attn_local / mc_block_attn_round): the remaining gather rounds
    attn_chain_open(e, layer);
    while (e->attn_rounds_done < sp_rounds(e)) MC_TRY(sp_attn_launch(e, layer, e->attn_rounds_done, s));
    e->attn_layer = -2;
  }
  {  // x = x + o(attn) * e[2]
    Prof pr(e, MC_PROF_GEMM_O, s);
    mc::GemmParams p = {};
    p.X = x; p.ldx = d; p.gate = em + 2 * d;
    if (em2) { p.gate2 = em2 + 2 * d; p.gate_sel = sel; }
    gate_table(e, p);
    MC_TRY(linear(e, l.o, whole(l.o), Lp, ActSrc{ao, d}, p, mc::EPI_RESID_GATE, s));
  }
  // ---- cross attention: x = x + o(attn(norm_q(q(norm3(x))), norm_k(k(ctx)), v(ctx)))
  ActSrc xn;   // LayerNorm output: the activation rows of cross-attention Q
  {
    Prof pr(e, MC_PROF_LN_MODULATE, s);
    MC_TRY(ln_for_gemm(e, l.cq, x, l.n3w, l.n3b, 1, nullptr, nullptr, nullptr, s, &xn));
  }
  {
    Prof pr(e, MC_PROF_GEMM_CROSS_Q, s);
    MC_TRY(linear_bf16_out(e, l.cq, Lp, xn, cq, mc::EPI_BF16, s));
  }
  Prof pr(e, MC_PROF_RMSNORM_ROPE, s);
  HIP_TRY(mc::launch_rmsnorm_rope(cq, d, l.cnq, e->cfg.eps, nullptr, 0, Lp, d, s));
  return MC_OK;
}

// MagCache residual capture (residual = x_out - ori_x, :299-301), the one place that knows where the residual of
// (branch, mode) goes and what follows once it is there.  Who writes it differs: the fused epilogue of the last FFN-2
// (block_post_ctx), or a separate launch_residual_sub where the last layer still receives a VACE hint (capture_unfused).
// A calibration forward writes the scratch slot, compares it with the branch's previous residual and swaps the two.
static float* capture_dst(const mc_engine* e, int branch, mc_mode mode) {
  return e->residual(mode == MC_MODE_CALIB ? e->res_scratch : e->res_slot[branch]);
}
// timed: the statistics launch is logged as MC_PROF_OTHER (the fused path; the unfused one never was)
static mc_status capture_written(mc_engine* e, int branch, mc_mode mode, bool timed, hipStream_t s) {
  const int d = e->d;
  if (mode == MC_MODE_CALIB) {
    if (!e->cfg.calibration) return fail(MC_ESTATE, "engine was created without calibration=1");
    if (e->have_res[branch]) {
      Prof pr(e, timed ? MC_PROF_OTHER : -1, s);
      HIP_TRY(mc::launch_calib_stats(e->residual(e->res_scratch), d, e->residual(e->res_slot[branch]), d, e->Lr, d,
                                     e->buf<double>("calib_partial"), 2048, e->buf<double>("calib_sums"),
                                     e->buf<float>("calib_stats") + 3 * branch, s));
    }
    e->have_stats[branch] = e->have_res[branch];
    std::swap(e->res_slot[branch], e->res_scratch);
  }
  e->have_res[branch] = true;
  return MC_OK;
}

static mc_status block_post_ctx(mc_engine* e, const Layer& l, const float* em, float* x, const bf16_t* cq, bool capture,
                                int branch, mc_mode mode, hipStream_t s) {
  const int d = e->d, Lp = e->Lp, ffn = e->ffn;
  bf16_t* ao = e->buf<bf16_t>("ao");
  const float* em2 = second_set(e, em);
  const uint8_t* sel = tok_sel(e);
  bf16_t* ckv = e->buf<bf16_t>("ckv");
  {
    if (e->ctx_active >= 0) {
      // constant over a video for this context: computed once by mc_set_context
      ckv = e->buf<bf16_t>("ckv_cache") + ((size_t)e->ctx_active * (e->NL + e->NV) + l.index) * e->ctx_rows * 2 * d;
    } else {
      Prof pr(e, MC_PROF_OTHER, s);
      MC_TRY(context_kv(e, l, e->buf<bf16_t>("ctx"), ckv, s));
    }
    {
      Prof pr(e, MC_PROF_ATTN_CROSS, s);
      MC_TRY(attend(e, cq, d, ao, kv_pairs(ckv, d, e->ctx_rows, e->cfg.text_len), nullptr, nullptr, s));
    }
    if (e->cfg.clip_dim > 0) {
      Prof pr(e, MC_PROF_OTHER, s);
      // I2V (upstream WanI2VCrossAttention): + attention over the 257 CLIP image tokens with their own k/v
      bf16_t* ckvi = e->buf<bf16_t>("ckv_img");
      bf16_t* ao2 = e->buf<bf16_t>("ao2");
      MC_TRY(linear_bf16_out(e, l.ckv_img, e->img_rows, ActSrc{e->buf<bf16_t>("ctx_img"), d}, ckvi, mc::EPI_BF16, s));
      HIP_TRY(mc::launch_rmsnorm_rope(ckvi, 2 * d, l.cnk_img, e->cfg.eps, nullptr, 0, e->img_rows, d, s));
      MC_TRY(attend(e, cq, d, ao2, kv_pairs(ckvi, d, e->img_rows, 257), nullptr, nullptr, s));
      HIP_TRY(mc::launch_add_bf16(ao, ao2, (size_t)Lp * d, s));
    }
    Prof pr(e, MC_PROF_GEMM_CROSS_O, s);
    mc::GemmParams o = {};
    o.X = x; o.ldx = d; o.gate = nullptr;
    MC_TRY(linear(e, l.co, whole(l.co), Lp, ActSrc{ao, d}, o, mc::EPI_RESID_GATE, s));
  }
  // ---- FFN: x = x + ffn(LN(x)*(1+e[4])+e[3]) * e[5]
  ActSrc xn;   // LayerNorm output: the activation rows of FFN-1
  {
    Prof pr(e, MC_PROF_LN_MODULATE, s);
    MC_TRY(ln_for_gemm(e, l.ffn1, x, em + 4 * d, em + 3 * d, 0, em2 ? em2 + 4 * d : nullptr, em2 ? em2 + 3 * d : nullptr, sel,
                       s, &xn, set_stride(e)));
  }
  bf16_t* h = e->buf<bf16_t>("h");
  mc::GemmParams p = {};
  p.Cb = h; p.ldc = ffn;
  // MX with fused quantisers: FFN-1's GELU epilogue writes the e4m3 rows + block scales FFN-2 reads (both inside "h":
  // Lp * ffn bytes, then ffn / 32 * Lp scale bytes), the bf16 hidden tensor never exists
  const bool h_fp8 = l.ffn1.mx && l.ffn2.mx && fused_quant(l.ffn1);
  ActSrc hidden{h, ffn};
  if (h_fp8) {
    hidden.quantised = true; hidden.q = (uint8_t*)h; hidden.mx = hidden.q + (size_t)Lp * ffn;
    p.Cq = hidden.q; p.ldcq = ffn; p.c_mx = hidden.mx; p.mx_rows_c = Lp;
  }
  {
    Prof pr(e, MC_PROF_GEMM_FFN1, s);
    MC_TRY(linear(e, l.ffn1, whole(l.ffn1), Lp, xn, p, h_fp8 ? mc::EPI_GELU_MXFP8 : mc::EPI_GELU_BF16, s));
  }
  mc::GemmParams q = {};
  q.X = x; q.ldx = d; q.gate = em + 5 * d;
  if (e->splitk_bytes) { q.splitk_ws = e->buf<float>("splitk"); q.splitk_ws_bytes = e->splitk_bytes; }
  if (em2) { q.gate2 = em2 + 5 * d; q.gate_sel = sel; }
  gate_table(e, q);
  if (capture) {   // fused into the last epilogue
    q.X0 = e->buf<bf16_t>("x0"); q.ldx0 = d;
    q.R = capture_dst(e, branch, mode); q.ldr = d;
  }
  {
    Prof pr(e, MC_PROF_GEMM_FFN2, s);
    MC_TRY(linear(e, l.ffn2, whole(l.ffn2), Lp, hidden, q, capture ? mc::EPI_RESID_CAPTURE : mc::EPI_RESID_GATE, s));
  }
  return capture ? capture_written(e, branch, mode, true, s) : MC_OK;
}

static mc_status block_post(mc_engine* e, const Layer& l, const float* em, float* x, int layer, bf16_t* cq, bool capture,
                            int branch, mc_mode mode, hipStream_t s) {
  MC_TRY(block_post_self(e, l, em, x, layer, cq, s));
  return block_post_ctx(e, l, em, x, cq, capture, branch, mode, s);
}

// The last main layer receives a VACE hint: no fused capture there, the residual is taken after the hint was added.
static bool hint_on_last_layer(const mc_engine* e) {
  return e->NV > 0 && (e->NV - 1) * e->cfg.vace_stride == e->NL - 1;
}

mc_status mc_block_post_attn(mc_engine* e, int layer, int branch, mc_mode mode, mc_stream stream_) {
  if (!e || !e->embedded) return fail(MC_ESTATE, "mc_embed must run first");
  if (layer < 0 || layer >= e->NL) return fail(MC_EINVAL, "layer %d out of range", layer);
  if (branch < 0 || branch >= e->cfg.n_branches) return fail(MC_EINVAL, "branch %d out of range", branch);
  e->pair_drop();
  return block_post(e, e->layers[layer], e->emod(e->layers[layer]), e->buf<float>("x"), layer, e->buf<bf16_t>("qkv"),
                    layer == e->NL - 1 && !hint_on_last_layer(e), branch, mode, (hipStream_t)stream_);
}

// VACE: control block i on the stream c, then x += after_proj(c) * context_scale (the "hint" of main layer
// i * vace_stride; upstream VaceWanAttentionBlock / BaseWanAttentionBlock, reference call site :544-549)
static mc_status vace_pre_kv(mc_engine* e, int i, hipStream_t s) {
  const int d = e->d, Lp = e->Lp;
  float* xc = e->buf<float>("xc");
  if (i == 0) {
    // c = before_proj(c0) + x, x = the embedded latent (ori_x, bf16 under autocast)
    HIP_TRY(hipMemsetAsync(xc, 0, (size_t)Lp * d * 4, s));
    HIP_TRY(mc::launch_skip_add(e->buf<bf16_t>("x0"), d, xc, d, xc, d, Lp, d, s));
    mc::GemmParams p = {};
    p.X = xc; p.ldx = d; p.gate = nullptr;
    MC_TRY(linear(e, e->before, whole(e->before), Lp, ActSrc{e->buf<bf16_t>("c0"), d}, p, mc::EPI_RESID_GATE, s));
  }
  return block_pre_kv(e, e->vlayers[i], e->emod(e->vlayers[i]), xc, s);
}

static mc_status vace_pre(mc_engine* e, int i, hipStream_t s) {
  MC_TRY(vace_pre_kv(e, i, s));
  return block_pre_q(e, e->vlayers[i], s);
}

static mc_status vace_post(mc_engine* e, int i, int branch, mc_mode mode, hipStream_t s) {
  const int d = e->d, Lp = e->Lp;
  float* xc = e->buf<float>("xc");
  MC_TRY(block_post(e, e->vlayers[i], e->emod(e->vlayers[i]), xc, -1, e->buf<bf16_t>("qkv"), false, branch, mode, s));
  // hint: after_proj(c) needs bf16 rows of c; the LayerNorm scratch xn is free here
  bf16_t* xn = e->buf<bf16_t>("xn");
  HIP_TRY(mc::launch_cast_bf16(xc, xn, (size_t)Lp * d, s));
  mc::GemmParams h = {};
  h.X = e->buf<float>("x"); h.ldx = d; h.gate = e->vscale;
  return linear(e, e->after[i], whole(e->after[i]), Lp, ActSrc{xn, d}, h, mc::EPI_RESID_GATE, s);
}

static mc_status vace_block(mc_engine* e, int i, int branch, mc_mode mode, hipStream_t s) {
  MC_TRY(vace_pre(e, i, s));
  return vace_post(e, i, branch, mode, s);
}

// Sequence parallel: control block i in two phases, like the main blocks (the caller all-gathers "kv_gather" between
// them).  Main layer i * vace_stride must have completed its block_post before vace_block_post(i) adds the hint.
mc_status mc_vace_block_pre(mc_engine* e, int i, mc_stream stream) {
  if (!e || !e->embedded) return fail(MC_ESTATE, "mc_embed must run first");
  if (i < 0 || i >= e->NV) return fail(MC_EINVAL, "VACE block %d out of range", i);
  if (!e->have_vace) return fail(MC_ESTATE, "mc_set_vace_context must run first");
  return vace_pre(e, i, (hipStream_t)stream);
}

mc_status mc_vace_block_post(mc_engine* e, int i, int branch, mc_mode mode, mc_stream stream) {
  if (!e || !e->embedded) return fail(MC_ESTATE, "mc_embed must run first");
  if (i < 0 || i >= e->NV) return fail(MC_EINVAL, "VACE block %d out of range", i);
  if (branch < 0 || branch >= e->cfg.n_branches) return fail(MC_EINVAL, "branch %d out of range", branch);
  return vace_post(e, i, branch, mode, (hipStream_t)stream);
}

// Sequence parallel, the layer loop in ONE call.  With C = mc_sp_set_chunks rounds (R of them carry valid keys), for every
// layer in [layer_begin, layer_end):
//   pre_kv                                  [LayerNorm, k|v Linear -> "kv_local", k norm / RoPE: what the peers wait for]
//   gather(user, layer, 2 c, stream)        c = 0 .. R-1: the caller STARTS round c of its all-gather (rows
//                                           [c Lp/C, (c+1) Lp/C) of "kv_local" -> "kv_gather"[c]) on its own communicator,
//                                           ordered behind what `stream` holds
//   pre_q, attn_local                       [q Linear + norm / RoPE, this rank's shard: beside the gather]
//   gather(user, layer, 2 c + 1, stream)    the caller makes `stream` wait for round c (no host sync) ...
//   attn_round c                            ... and the attention over it runs while round c + 1 is on the wire
//   post_attn                               (+ the VACE control block of that layer in the same phases, with its own gather)
// overlap == 0: every wait comes right after the starts -- nothing runs beside the collective (the A/B baseline).
// The phase argument of C = 1 is the 0 / 1 (start / wait) of the unchunked protocol.  The waits are bracketed as
// MC_PROF_SP_WAIT: with mc_profile_enable(2) their summed time is what the launch stream idled for the collective.
// mc_block_pre_kv / _pre_q / _attn_local / _attn_round / _post_attn stay exported: same code underneath.
mc_status mc_blocks_sp(mc_engine* e, int layer_begin, int layer_end, int branch, mc_mode mode, int overlap,
                       mc_sp_gather_fn gather, void* user, mc_stream stream) {
  if (!e || !e->embedded) return fail(MC_ESTATE, "mc_embed must run first");
  if (!gather) return fail(MC_EINVAL, "null gather callback");
  if (!e->sp) return fail(MC_ESTATE, "mc_blocks_sp needs a sequence-parallel engine (sp_size > 1 or sp_phases) (one GPU: mc_forward)");
  if (layer_begin < 0 || layer_end > e->NL || layer_begin > layer_end)
    return fail(MC_EINVAL, "layers [%d, %d) out of range (num_layers %d)", layer_begin, layer_end, e->NL);
  if (mode == MC_MODE_SKIP) return fail(MC_EINVAL, "a skipped forward runs no blocks (mc_embed -> mc_head)");
  hipStream_t s = (hipStream_t)stream;
  const int R = sp_rounds(e);
  auto coll = [&](int layer, int phase) -> mc_status {
    const int rc = gather(user, layer, phase, stream);
    return rc == 0 ? MC_OK : fail(MC_ESTATE, "gather callback failed (layer %d, phase %d, code %d)", layer, phase, rc);
  };
  auto wait_round = [&](int layer, int c, hipStream_t on) -> mc_status {
    Prof pr(e, MC_PROF_SP_WAIT, on);
    const int rc = gather(user, layer, 2 * c + 1, (mc_stream)on);
    return rc == 0 ? MC_OK : fail(MC_ESTATE, "gather callback failed (layer %d, phase %d, code %d)", layer, 2 * c + 1, rc);
  };
  // independent partial launches on two streams + one merge (see g_sp_attn_partials); a world of one has nothing to merge
  if (!g_n_cu) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      g_n_cu = n;
    else
      g_n_cu = 256;
  }
  // one workgroup = 256 query rows of one head = one CU: the launch runs in ceil(wg / CUs) waves of which the last is partial
  const long wg = (long)(e->Lp / 256) * e->H, waves = (wg + g_n_cu - 1) / g_n_cu;
  const bool underfilled = wg * 10 < waves * g_n_cu * 9;               // < 90 % of the CU slots it occupies (sp 4 / 8 at 1.3B: 75 %;
                                                                       // 14B at sp 8: 1480 workgroups = 96 %: the merge would only cost)
  const bool partials = (mc::g_sp_attn_partials == 2 || (mc::g_sp_attn_partials == 1 && underfilled)) && e->P > 1 && 1 + R <= kSpMaxParts;
  if (partials) MC_TRY(sp_side_stream(e));
  // one attention chain: starts, [waits], q, local shard, ([wait] round) x R
  auto chain = [&](int l, const Layer& ly, int chain_id) -> mc_status {
    for (int c = 0; c < R; ++c) MC_TRY(coll(l, 2 * c));
    if (!overlap)
      for (int c = 0; c < R; ++c) MC_TRY(wait_round(l, c, s));
    MC_TRY(block_pre_q(e, ly, s));
    if (!partials) {
      MC_TRY(sp_attn_launch(e, chain_id, -1, s));
      for (int c = 0; c < R; ++c) {
        if (overlap) MC_TRY(wait_round(l, c, s));
        MC_TRY(sp_attn_launch(e, chain_id, c, s));
      }
      return MC_OK;
    }
    // ONE event pair on the launch stream around the whole chain (fork .. join .. merge): its launches overlap on two streams,
    // pairs around each would count the shared time twice.  Stalls for gather rounds are inside it AND logged as SP_WAIT.
    Prof chain_pr(e, MC_PROF_ATTN_SELF, s);
    // q is ready (and the previous layer's merge has read the partial slots) once `s` gets here: the side stream follows
    HIP_TRY(hipEventRecord(e->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(e->side, e->ev_fork, 0));
    MC_TRY(sp_attn_partial(e, -1, s));
    for (int c = 0; c < R; ++c) {
      hipStream_t on = (c & 1) ? s : e->side;          // round 0 beside the local shard, then alternating
      if (overlap) MC_TRY(wait_round(l, c, on));
      MC_TRY(sp_attn_partial(e, c, on));
    }
    HIP_TRY(hipEventRecord(e->ev_join, e->side));
    HIP_TRY(hipStreamWaitEvent(s, e->ev_join, 0));
    const bf16_t* op[kSpMaxParts];
    const float* lp[kSpMaxParts];
    for (int i = 0; i <= R; ++i) {
      op[i] = e->buf<bf16_t>("ao_part") + (size_t)i * e->Lp * e->d;
      lp[i] = e->buf<float>("lse_part") + (size_t)i * e->H * e->Lp;
    }
    HIP_TRY(mc::launch_attn_merge(op, lp, 1 + R, e->buf<bf16_t>("ao"), e->d, e->Lp, e->Lp, e->d, s));
    // the chain is complete: block_post has nothing left to attend
    attn_chain_set(e, chain_id, 1 + R, true, R);
    return MC_OK;
  };
  for (int l = layer_begin; l < layer_end; ++l) {
    MC_TRY(block_pre_kv(e, e->layers[l], e->emod(e->layers[l]), e->buf<float>("x"), s));
    MC_TRY(chain(l, e->layers[l], l));
    MC_TRY(mc_block_post_attn(e, l, branch, mode, stream));
    if (e->NV > 0 && l % e->cfg.vace_stride == 0 && l / e->cfg.vace_stride < e->NV) {
      const int i = l / e->cfg.vace_stride;
      if (!e->have_vace) return fail(MC_ESTATE, "mc_set_vace_context must run first");
      MC_TRY(vace_pre_kv(e, i, s));
      MC_TRY(chain(l, e->vlayers[i], -1));
      MC_TRY(mc_vace_block_post(e, i, branch, mode, stream));
    }
  }
  return MC_OK;
}

// residual capture as a separate kernel (only when the last layer carries a VACE hint)
static mc_status capture_unfused(mc_engine* e, int branch, mc_mode mode, hipStream_t s) {
  const int d = e->d;
  HIP_TRY(mc::launch_residual_sub(e->buf<float>("x"), d, e->buf<bf16_t>("x0"), d, capture_dst(e, branch, mode), d, e->Lp, d, s));
  return capture_written(e, branch, mode, false, s);
}

// head(x, e) on this rank's tokens -> "head_tokens" [Lr, 4*out_dim] fp32       (reference :304)
static mc_status head(mc_engine* e, const float* x, int branch, mc_mode mode, hipStream_t s) {
  if (!e || !e->embedded) return fail(MC_ESTATE, "mc_embed must run first");
  if (branch < 0 || branch >= e->cfg.n_branches) return fail(MC_EINVAL, "branch %d out of range", branch);
  const int d = e->d;
  const float* eh = e->buf<float>("ehead");
  const float* eh2 = e->tok_t && !e->cfg.token_timestep_sets ? eh + 2 * d : nullptr;
  const uint8_t* sel = tok_sel(e);
  const long hst = e->tok_t && e->cfg.token_timestep_sets ? 2 * d : 0;   // a capacity engine: "ehead" is a table of C sets
  const int hsets = hst ? e->cfg.token_timestep_sets : 0;
  float* hn = e->buf<float>("h");
  Prof pr(e, MC_PROF_HEAD, s);
  if (mode == MC_MODE_SKIP) {
    // skipped step: x = ori_x + residual_cache[branch] (:294-295), folded into the LayerNorm load
    if (!e->have_res[branch]) return fail(MC_ESTATE, "skip requested but residual_cache[%d] is empty", branch);
    HIP_TRY(mc::launch_ln_modulate(e->residual(e->res_slot[branch]), d, e->buf<bf16_t>("x0"), d, eh + d, eh, 0,
                                   e->cfg.eps, nullptr, 0, hn, d, e->Lr, d, s, eh2 ? eh2 + d : nullptr, eh2, sel, hst, hsets));
  } else {
    HIP_TRY(mc::launch_ln_modulate(x, d, nullptr, 0, eh + d, eh, 0, e->cfg.eps, nullptr, 0, hn, d,
                                   e->Lr, d, s, eh2 ? eh2 + d : nullptr, eh2, sel, hst, hsets));
  }
  HIP_TRY(mc::launch_head_linear(hn, d, e->w_head, e->b_head, e->buf<float>("head_tokens"), e->HT, e->Lr,
                                 e->cfg.out_dim * 4, d, s));
  return MC_OK;
}

mc_status mc_head(mc_engine* e, int branch, mc_mode mode, mc_stream stream) {
  if (!e) return fail(MC_ESTATE, "mc_embed must run first");
  e->pair_drop();   // every phase call ends a declared pair: between its forwards "x" is not a finished stream
  e->phase_open = false;
  return head(e, e->buf<float>("x"), branch, mode, (hipStream_t)stream);
}

mc_status mc_unpatchify(mc_engine* e, const float* tokens_dev, int tok0, int n_tok, float* out_dev,
                        mc_stream stream_) {
  if (!e || !tokens_dev || !out_dev) return fail(MC_EINVAL, "null argument");
  if (tok0 < 0 || n_tok <= 0 || tok0 + n_tok > e->L) return fail(MC_EINVAL, "token range out of bounds");
  const mc_config& c = e->cfg;
  Prof pr(e, MC_PROF_HEAD, (hipStream_t)stream_);
  HIP_TRY(mc::launch_unpatchify(tokens_dev, e->HT, c.out_dim, c.latent_f, c.latent_h, c.latent_w, tok0, n_tok, out_dev,
                                (hipStream_t)stream_));
  return MC_OK;
}

// CFG pair.  The sampler evaluates the model twice per step on the same latent and the same t; only the text context differs,
// and the context first enters a block at layer 0's cross-attention K|V.  Between mc_pair_begin and mc_pair_end the first
// mc_forward that runs its blocks works on "pair_x" / "pair_cq" instead of "x" / "qkv" and copies the stream to "x" behind
// layer 0's O epilogue (the epilogues update the stream in place: one of the two forwards needs its own copy); the second
// starts from that "x" at layer 0's cross-attention.  The same kernels run on the same values in the same order as in two
// full forwards, so the results are the same bits.
mc_status mc_pair_begin(mc_engine* e) {
  if (!e) return fail(MC_EINVAL, "null engine");
  e->pair = e->pair_capable() ? mc_engine::PAIR_ARMED : mc_engine::PAIR_NONE;
  return MC_OK;
}

mc_status mc_pair_end(mc_engine* e) {
  if (!e) return fail(MC_EINVAL, "null engine");
  e->pair = mc_engine::PAIR_NONE;
  return MC_OK;
}

// the forward behind mc_forward's argument checks; a failure leaves the pair state to the caller
static mc_status forward(mc_engine* e, const float* latent_dev, const float* t_dev, double t_host, const void* context_dev,
                         mc_dtype ctx_dtype, int ctx_len, int branch, mc_mode mode, float* out_dev, hipStream_t s) {
  const int d = e->d;
  // this call's place in a declared pair: `keep` = it runs the front and leaves it behind, `reuse` = it continues from the
  // front the call before it left.  Every other case -- a skipped forward on either side, another t, a third forward -- ends
  // the sharing, and the call runs in full
  const bool runs = mode != MC_MODE_SKIP;
  const bool reuse = e->pair == mc_engine::PAIR_KEPT && runs && latent_dev == e->pair_latent && t_dev == e->pair_t_dev &&
                     t_host == e->pair_t_host;
  const bool keep = e->pair == mc_engine::PAIR_ARMED && runs;
  e->pair = keep ? mc_engine::PAIR_KEPT : e->pair == mc_engine::PAIR_NONE ? mc_engine::PAIR_NONE : mc_engine::PAIR_DEAD;
  if (keep) { e->pair_latent = latent_dev; e->pair_t_dev = t_dev; e->pair_t_host = t_host; }
  float* x = e->buf<float>(keep ? "pair_x" : "x");
  bf16_t* cq = e->buf<bf16_t>(keep || reuse ? "pair_cq" : "qkv");
  if (reuse) {
    MC_TRY(check_ready(e));
    Prof pr(e, context_dev ? MC_PROF_EMBED : -1, s);
    MC_TRY(embed_text(e, context_dev, ctx_dtype, ctx_len, s));
  } else {
    MC_TRY(embed(e, latent_dev, t_dev, t_host, context_dev, ctx_dtype, ctx_len, x, s));
  }
  for (int l = 0; runs && l < e->NL; ++l) {
    const Layer& ly = e->layers[l];
    const float* em = e->emod(ly);
    bf16_t* lcq = l == 0 ? cq : e->buf<bf16_t>("qkv");
    if (!(reuse && l == 0)) {
      MC_TRY(block_pre(e, ly, em, x, s));
      MC_TRY(block_post_self(e, ly, em, x, l, lcq, s));
    }
    if (keep && l == 0) {
      Prof pr(e, MC_PROF_OTHER, s);
      if (hipMemcpyAsync(e->buf<float>("x"), x, (size_t)e->Lp * d * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return fail(MC_EHIP, "hipMemcpyAsync of the kept stream failed");
    }
    MC_TRY(block_post_ctx(e, ly, em, x, lcq, l == e->NL - 1 && !hint_on_last_layer(e), branch, mode, s));
    if (e->NV > 0 && l % e->cfg.vace_stride == 0 && l / e->cfg.vace_stride < e->NV)
      MC_TRY(vace_block(e, l / e->cfg.vace_stride, branch, mode, s));
  }
  if (runs && hint_on_last_layer(e)) MC_TRY(capture_unfused(e, branch, mode, s));
  MC_TRY(head(e, x, branch, mode, s));
  return mc_unpatchify(e, e->buf<float>("head_tokens"), 0, e->L, out_dev, (mc_stream)s);
}

mc_status mc_forward(mc_engine* e, const float* latent_dev, const float* t_dev, double t_host,
                     const void* context_dev, mc_dtype ctx_dtype, int ctx_len, int branch, mc_mode mode,
                     float* out_dev, mc_stream stream) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->sp) return fail(MC_ESTATE, "mc_forward is single-GPU; drive a sharded engine through the phase calls");
  if (!out_dev) return fail(MC_EINVAL, "null output");
  if (e->NV > 0 && mode != MC_MODE_SKIP && !e->have_vace)
    return fail(MC_ESTATE, "VACE model: mc_set_vace_context must run before a non-skipped forward");
  if (branch < 0 || branch >= e->cfg.n_branches) return fail(MC_EINVAL, "branch %d out of range", branch);
  const mc_status st = forward(e, latent_dev, t_dev, t_host, context_dev, ctx_dtype, ctx_len, branch, mode, out_dev,
                               (hipStream_t)stream);
  if (st != MC_OK) e->pair_drop();   // whatever failed: a kept front is not continued from
  return st;
}

mc_status mc_calib_ready(const mc_engine* e, int branch, int* has_stats) {
  if (!e || !has_stats || branch < 0 || branch > 1) return fail(MC_EINVAL, "bad argument");
  *has_stats = e->have_stats[branch] ? 1 : 0;
  return MC_OK;
}

mc_status mc_calib_finalize(mc_engine* e, int branch, mc_stream stream) {
  if (!e || !e->work.ws) return fail(MC_ESTATE, "no workspace");
  if (branch < 0 || branch > 1) return fail(MC_EINVAL, "branch %d out of range", branch);
  HIP_TRY(mc::launch_calib_finalize(e->buf<double>("calib_sums"), e->buf<float>("calib_stats") + 3 * branch,
                                    (hipStream_t)stream));
  return MC_OK;
}

mc_status mc_import_residual(mc_engine* e, int branch, const float* src_dev, mc_stream stream) {
  if (!e || !e->work.ws || !src_dev) return fail(MC_EINVAL, "null argument / no workspace");
  if (branch < 0 || branch >= e->cfg.n_branches) return fail(MC_EINVAL, "branch %d out of range", branch);
  float* dst = e->residual(e->res_slot[branch]);
  if (dst != src_dev)
    HIP_TRY(hipMemcpyAsync(dst, src_dev, (size_t)e->Lr * e->d * sizeof(float), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
  e->have_res[branch] = true;
  return MC_OK;
}

mc_status mc_set_context(mc_engine* e, int slot, const void* context_dev, mc_dtype ctx_dtype, int ctx_len,
                         mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  MC_TRY(check_ready(e));
  if (slot < 0 || slot > 1) return fail(MC_EINVAL, "context slot %d out of range (0, 1)", slot);
  if (e->cfg.no_context_cache) return fail(MC_ESTATE, "the engine was created with no_context_cache: pass the context to every forward");
  if (!context_dev) return fail(MC_EINVAL, "null context");
  const int d = e->d;
  bf16_t* ctx = e->buf<bf16_t>("ctx_cache") + (size_t)slot * e->ctx_rows * d;
  e->ctx_valid[slot] = false;
  MC_TRY(embed_context(e, context_dev, ctx_dtype, ctx_len, ctx, s));
  bf16_t* base = e->buf<bf16_t>("ckv_cache") + (size_t)slot * (e->NL + e->NV) * e->ctx_rows * 2 * d;
  for (int l = 0; l < e->NL + e->NV; ++l) MC_TRY(context_kv(e, e->layer(l), ctx, base + (size_t)l * e->ctx_rows * 2 * d, s));
  e->ctx_valid[slot] = true;
  e->ctx_active = slot;
  return MC_OK;
}

mc_status mc_use_context(mc_engine* e, int slot) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (slot < -1 || slot > 1) return fail(MC_EINVAL, "context slot %d out of range (-1, 0, 1)", slot);
  if (slot >= 0 && e->cfg.no_context_cache) return fail(MC_ESTATE, "the engine was created with no_context_cache");
  if (slot >= 0 && !e->ctx_valid[slot]) return fail(MC_ESTATE, "context slot %d was never set (mc_set_context)", slot);
  e->ctx_active = slot;
  return MC_OK;
}

mc_status mc_set_token_timesteps(mc_engine* e, const float* t_tokens_dev, mc_stream) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (t_tokens_dev && e->NV > 0) return fail(MC_EINVAL, "per-token timesteps are not defined for the VACE model");
  if (t_tokens_dev && e->cfg.no_token_timesteps) return fail(MC_ESTATE, "the engine was created with no_token_timesteps");
  e->tok_t = t_tokens_dev;
  e->pair_drop();   // the modulation sets of a kept front belong to the timesteps it was embedded with
  return MC_OK;
}

mc_status mc_profile_enable(mc_engine* e, int on) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (on < 0 || on > 2) return fail(MC_EINVAL, "profile level %d (0 off, 1 self-attention, 2 every class)", on);
  if (on && e->prof_ev.empty()) {
    e->prof_ev.resize(2 * 8192);
    e->prof_cls.assign(8192, 0);
    for (auto& ev : e->prof_ev) HIP_TRY(hipEventCreate(&ev));
  }
  e->profile = on;
  e->prof_n = 0;
  return MC_OK;
}

// waits for the logged pairs and sums them by class; clears the log
mc_status mc_profile_read_classes(mc_engine* e, double ms_total[MC_PROF_NCLASS], int launches[MC_PROF_NCLASS]) {
  if (!e || !ms_total || !launches) return fail(MC_EINVAL, "null argument");
  for (int c = 0; c < MC_PROF_NCLASS; ++c) { ms_total[c] = 0.0; launches[c] = 0; }
  const size_t n = e->prof_n;
  e->prof_n = 0;
  for (size_t i = 0; i + 1 < n; i += 2) {
    const int c = e->prof_cls[i / 2];
    if (c >= MC_PROF_NCLASS) continue;       // a pair whose second record failed
    HIP_TRY(hipEventSynchronize(e->prof_ev[i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->prof_ev[i], e->prof_ev[i + 1]));
    ms_total[c] += ms;
    launches[c] += 1;
  }
  return MC_OK;
}

mc_status mc_profile_read(mc_engine* e, double* attn_ms_total, int* attn_launches) {
  if (!e || !attn_ms_total || !attn_launches) return fail(MC_EINVAL, "null argument");
  double ms[MC_PROF_NCLASS];
  int n[MC_PROF_NCLASS];
  MC_TRY(mc_profile_read_classes(e, ms, n));
  *attn_ms_total = ms[MC_PROF_ATTN_SELF];
  *attn_launches = n[MC_PROF_ATTN_SELF];
  return MC_OK;
}

mc_status mc_state_reset(mc_engine* e) {
  if (!e) return fail(MC_EINVAL, "null engine");
  e->have_res[0] = e->have_res[1] = false;
  e->have_stats[0] = e->have_stats[1] = false;
  return MC_OK;
}

mc_status mc_op_rope_table(int F, int Hp, int Wp, int tok0, int n_tok, float* cs_host) {
  if (!cs_host || n_tok <= 0) return fail(MC_EINVAL, "bad argument");
  rope_table_host(F, Hp, Wp, tok0, n_tok, cs_host);
  return MC_OK;
}

mc_status mc_op_rope_axes(int F, int Hp, int Wp, float* axes_host, size_t* n_floats) {
  if (F <= 0 || Hp <= 0 || Wp <= 0 || (!axes_host && !n_floats)) return fail(MC_EINVAL, "bad argument");
  if (n_floats) *n_floats = rope_axes_floats(F, Hp, Wp);
  if (axes_host) rope_axes_host(F, Hp, Wp, axes_host);
  return MC_OK;
}

}  // extern "C"
