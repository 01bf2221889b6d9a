// MM-DiT engine behind include/magcache_mmdit.h: FLUX.1 (diffusers FluxTransformer2DModel), HunyuanVideo
// (hyvideo HYVideoDiffusionTransformer) and Qwen-Image (diffusers QwenImageTransformer2DModel) forward with the MagCache
// skip path, on the kernels of this library.
//
// Reference boundary: the body of magcache_forward in MagCache4FLUX/magcache_flux.py:301-432,
// MagCache4HunyuanVideo/magcache_sample_video.py:40-146 and MagCache4QwenImage/magcache_generate.py:186-253; the blocks
// are upstream code (see oracle/flux_ref.py, oracle/hunyuan_ref.py and tests/qwen_image_ref.py for the restatements this
// engine is tested against).
//
// Qwen-Image (MC_FAMILY_QWEN) is FLUX's double block 60 times with no single blocks: rows [text ; image] like FLUX, the
// text rows sized for the longest prompt (txt_len) and the call's prompt in the first txt_valid of them.  The padded text
// rows [txt_valid, txt_len) are zero after txt_in (EPI_EMBED m_valid) and stay finite; they are left out of the key set
// by attending the image keys and the txt_valid text keys in two launches merged by their log-sum-exp (the sequence-
// parallel machinery), so the result is that of the unpadded sequence.  The two CFG branches keep their own residual
// slots (residual_cache[cnt % 2] of the reference).
//
// Data layout in HBM (one caller-owned workspace; d = dim, S = txt_len + img_tokens, S_pad = S up to 256):
//   x    fp32 [S_pad, d]    joint residual stream.  Row order = the family's attention order: FLUX [text ; image],
//                           HunyuanVideo [image ; text] -- the two streams of a double block are row ranges of it,
//                           so the single blocks need no concatenation (reference cat: flux :389, hunyuan :122)
//   x0   bf16 [S_pad, d]    ori_hidden_states / ori_img (flux :351, hunyuan :104) for the residual and the skip path;
//                           joint row index like x (only the image rows are meaningful)
//   xn   bf16 [S_pad, d]    LayerNorm + modulation output (GEMM operand)
//   qkv  bf16 [S_pad, 3d]   q | k | v of the joint sequence (attention reads it in place, strided)
//   am   bf16 [S_pad, 5d]   columns [0,d): attention output; [d,5d): GELU(MLP-in) -- exactly the operand of the
//                           single block's fused output projection (cat([attn, mlp]) upstream) with K = 5d
//   emod fp32               every block's modulation vector, produced by ONE bf16-weight GEMV over silu(vec)
//   residual0/1 fp32 [S_pad, d] MagCache residual cache (+ the previous one in calibration mode; Qwen-Image: per CFG
//                           branch, residual0..3 with calibration), joint row index: the
//                           capture is the epilogue of the LAST block's output GEMM (R = x_new - x0 per row); the image
//                           rows are the cache, the text rows are scratch
//   aq   packed [S_pad, 5d] (fp8_linear != 0 only) the quantised operand rows of the MX Linears, joint row index, columns as
//                           "am": [0,d) the LayerNorm + modulate output (q|k|v, MLP-in, the single block's linear1) and, mode
//                           3, the attention output (the output projections); [d,5d) GELU(MLP-in), MLP-out's operand
//                           in the engine's element format (ops.h: MxFormat; e4m3, or e2m1 / e2m3 with the option "mx_fp4" /
//                           "mx_fp6"): rows of mx_row_bytes(fmt, 5d) bytes, column c (a multiple of 32) at byte mx_row_bytes(fmt, c)
//   a_mx E8M0               (fp8_linear != 0 only) the block scales of "aq".  A scale image is block-major [k / 32][rows_pad]
//                           with the rows of every group of 64 interleaved RELATIVE TO THE LAUNCH'S FIRST ROW, so two row
//                           ranges must not share one: three regions, [text | image | joint (the single blocks)], each
//                           rows_pad = ceil256(rows of the range) long per k block and 5d/32 k blocks deep in "aq"'s column
//                           order (block d/32 starts the GELU columns); mode 3 adds d/32 blocks behind them in the text and
//                           the image region for the rows the output projections read (the single block's K = 5d output
//                           projection reads the joint region's whole image)
// GEMMs over one stream use the exact row count (the 256^2 kernel guards a partial last tile), so neighbouring
// rows of the other stream are never touched.
//
// Host structure (the Wan engine's, host.h): every weight matrix is an mc::Linear that WeightStore::add_linear allocates and
// registers under its upstream names; every GEMM goes through linear(), which takes operands and shape from the descriptor
// (a second Linear makes it the row-split launch over two row ranges); a double block is double_pre / double_post over one
// or two row ranges (Range) -- both streams in merged launches by default, one stream per call for the two-stream modes and
// sequence parallel; every attention launch is attend() over a key set (Keys).
// fp8_linear 2 / 3 (opt-in): the block Linears that read a LayerNorm or GELU output (3: the attention output too) keep an
// MX copy -- block scales, elements in the engine's MxFormat -- and run on launch_gemm_mx over the exact rows of ONE range (the
// kernels guard a partial last tile and have no row-split launch): a double block is then one pass per stream, in row order, on
// the launch stream.  The format is e4m3 unless the create call finds the option "mx_fp4" (W4A4, e2m1) or "mx_fp6" (W6A6, e2m3)
// set (host.h: latch_mx_format).  "aq" is written by the quantising tail of the LayerNorm kernel and MLP-in's quantising GELU
// epilogue (fp8_fused_quant 1; e4m3 and e2m1) or by launch_quantize_rows_mx (0, the attention output, and everything in e2m3,
// which has no fused producer: fused_quant below): the same bits either way.
#include <cmath>
#include <memory>

#include "../../include/magcache_mmdit.h"
#include "host.h"

using mc::align_up;
using mc::bf16_t;
using mc::fail;
using mc::Keys;
using mc::Linear;

namespace mc {
// mc_set_option("mmdit_two_streams", v): 0 = off (the DEFAULT since round 3: the packed-fp32 co-execution fault behind
// round 2's nondeterminism has a measured workaround but no root cause -- ADVICE r02 -- so the overlap is opt-in),
// -1 = by shape (on when the text half is at least 1/16 of the image half and the engine is not sequence parallel: FLUX),
// 1 on, 2..6 diagnostic splits (tests/two_stream_bisect.py)
int g_mmdit_two_streams = 0;
}  // namespace mc
using mc::g_mmdit_two_streams;

namespace {

struct Stream {  // one stream (image or text) of a double block
  Linear qkv, o, fc1, fc2;
  float *qn, *kn;
};
struct Single {
  Linear in, out;  // in = [q;k;v;mlp] rows [7d, d]; out [d, 5d]
  float *qn, *kn;
};
struct Mlp2 {  // Linear, SiLU, Linear on a vector
  Linear l1, l2;
};
struct Refiner {
  Linear qkv, o, fc1, fc2, ada;
  float *n1w, *n1b, *n2w, *n2b;
};
// One IP-Adapter (FLUX): diffusers' ImageProjection (Linear + affine LayerNorm) and, per double block, to_k_ip | to_v_ip as ONE
// Linear.  Two image slots (the positive and the negative image prompt of a true-CFG pipeline): the K|V of every double block
// for the slot's image, [n_double][rows][2d] bf16, computed once per image by mc_mmdit_ip_adapter_set_image.
struct IpAdapter {
  int embed_dim = 0, cross_dim = 0, tokens = 0;
  Linear proj;                       // [tokens * cross_dim, embed_dim]
  float *ln_w = nullptr, *ln_b = nullptr;
  std::vector<Linear> kv;            // per double block: [2d, cross_dim], rows to_k_ip | to_v_ip
  std::vector<float> scale;          // per double block
  bf16_t* cache[2] = {nullptr, nullptr};
  int keys[2] = {0, 0}, rows[2] = {0, 0};   // valid keys of the slot; rows allocated per block
  std::vector<std::string> names;    // what it registered in the store
};

}  // namespace

struct mc_mmdit {
  mc_mmdit_config cfg;
  int d, H, Li, Lt, S, Sp, Kin, Kp, img0, txt0, out_feat;   // Li = image tokens of THIS rank; S = Lt + Li
  int P = 1, rank = 0, tok0 = 0, Lrp = 0;                    // sequence parallel: image shard [tok0, tok0 + Li)
  mc_mode mode = MC_MODE_FULL;                               // of the forward in progress (begin .. end)
  int txt_valid = 0, dst = 0, local_attn_blk = -1;
  int branch = 0;                                            // CFG branch of the forward in progress (Qwen-Image: 0 / 1)
  bool begun = false;
  int fp8 = 0;                                               // cfg.fp8_linear: 0 | 2 | 3
  mc::MxFormat mx_fmt = mc::MX_E4M3;   // the element format of the MX Linears and of "aq" (fp8_linear 2 | 3), as the create call
                                       // latched it from the options "mx_fp4" / "mx_fp6" (host.h: latch_mx_format)
  // optional second compute stream: the text stream of a double block next to the image stream (mc_set_option
  // "mmdit_two_streams"); a ring of event pairs so that an event is not re-recorded while an earlier wait on it may
  // still be queued
  hipStream_t side = nullptr;
  hipEvent_t ev_fork[8] = {}, ev_join[8] = {};
  int ev_i = 0;
  size_t mod_rows = 0;  // rows of the fused modulation matrix
  std::vector<Stream> dimg, dtxt;
  std::vector<Single> singles;
  std::vector<Refiner> refiners;
  Mlp2 time_mlp, guid_mlp, vec_mlp, ref_t_mlp, ref_c_mlp;
  Linear img_in, txt_in, mod;   // image embedder [d, Kp], text embedder [d, txt_dim], fused modulation matrix [mod_rows, d]
  float *w_head = nullptr, *b_head = nullptr;
  float* w_txt_norm = nullptr;  // Qwen-Image txt_norm (RMSNorm over txt_dim)
  float* cs = nullptr;  // RoPE (cos,sin) [Sp][64][2]
  int cs_rows = 0;      // rows allocated behind cs (>= Sp: mc_mmdit_set_geometry grows it, never shrinks it)
  mc::WeightStore weights;
  mc::Workspace work;
  int res_cur[2] = {0, 0};  // per CFG branch: the slot (of the branch's own) holding residual_cache / previous_residual
  bool have_res[2] = {false, false}, have_stats = false, pads_clean = false;
  // ControlNet residuals (mc_mmdit_set_controlnet, FLUX): caller-owned [img_tokens, d] samples; host pointer lists only
  std::vector<const void*> cn_double, cn_single;
  mc_dtype cn_dtype = MC_F32;
  bool cn_repeat = false;
  // IP-Adapters (mc_mmdit_ip_adapter_*, FLUX): everything lives in the weight store, outside the workspace
  std::vector<std::unique_ptr<IpAdapter>> ip;   // (the store keeps pointers to the Linears: the adapters never move)
  int ip_slot = -1;                  // the image slot the forwards read; -1: none
  bf16_t* ip_out = nullptr;          // [Li, d]: the attention result of the block in progress
  int ip_out_rows = 0;
  float* ip_h32 = nullptr;           // set_image scratch: the projection [kIpMaxKeys, cross_dim] fp32 ...
  bf16_t* ip_hb = nullptr;           // ... and its LayerNorm, the operand of the K|V Linears
  int ip_h_cross = 0;

  template <class T>
  T* buf(const char* name) const { return work.get<T>(name); }
  // slot i (0 / 1) of CFG branch b: residual<b * slots_per_branch + i>; branch 0 is residual0 / residual1 as before
  int res_index(int b, int i) const { return b * (cfg.calibration ? 2 : 1) + i; }
  float* residual_joint(int i, int b = 0) const {
    static const char* nm[4] = {"residual0", "residual1", "residual2", "residual3"};
    return buf<float>(nm[res_index(b, i)]);
  }
  float* residual(int i, int b = 0) const { return residual_joint(i, b) + (size_t)img0 * d; }   // image rows
  size_t mod_double(int blk, int stream) const { return ((size_t)blk * 2 + stream) * 6 * d; }
  size_t mod_single(int blk) const { return (size_t)cfg.n_double * 12 * d + (size_t)blk * 3 * d; }
  size_t mod_final() const { return (size_t)cfg.n_double * 12 * d + (size_t)cfg.n_single * 3 * d; }
};

namespace {

// The packed rows [M, k_in] an MX Linear reads (ld bytes apart, mx_row_bytes of the Linear's format each), with their scale
// image (rows_pad >= ceil256(M) rows per k block)
struct MxRows {
  const uint8_t* q; long ld;
  const uint8_t* mx; long rows_pad;
};

// Every GEMM of the engine: y = epilogue(A l.w^T + l.b) over M rows, operands and shape from the descriptor, p carrying what
// the epilogue needs.  `lb` makes it the row-split launch over two row ranges of the same buffers: rows >= m_split use lb's
// weight and bias and gate_b.  The split-K scratch of the stream it runs on rides along (launch_gemm_bf16 decides by shape
// whether to use it: the projections back to d at FLUX sizes do, nothing at HunyuanVideo's 119 k tokens does).
// A Linear with an MX copy reads `a8` instead of A, over one row range (no lb); `out`: a range of its output channels (count
// 0 = all of them).
mc_status linear(const mc_mmdit* e, const Linear& l, int M, const bf16_t* A, long lda, mc::GemmParams p, int epi, hipStream_t s,
                 const Linear* lb = nullptr, int m_split = 0, const float* gate_b = nullptr, const MxRows* a8 = nullptr,
                 mc::RowRange out = {0, 0}) {
  if (out.count == 0) out = mc::whole(l);
  if (l.q) {
    if (!l.mx || !a8 || lb) return fail(MC_ESTATE, "an MX Linear runs over one row range of quantised rows");
    p.M = M; p.N = out.count; p.K = l.k_in; p.bias = l.b + out.first;
    p.A = (const bf16_t*)a8->q; p.lda = a8->ld; p.W = (const bf16_t*)(l.q + (size_t)out.first * l.q_row_bytes()); p.ldw = l.q_row_bytes();
    p.a_mx = a8->mx; p.mx_rows_a = a8->rows_pad; p.w_mx = l.mx + out.first; p.mx_rows_w = l.n_out;   // block-major: [k / 32][n_out]
    HIP_TRY(mc::launch_gemm_mx(l.fmt, p, epi, s));
    return MC_OK;
  }
  if (lb && lb->q) return fail(MC_ESTATE, "an MX Linear runs over one row range of quantised rows");
  const mc::Buf* b = e->work.find((e->side && s == e->side) ? "splitk1" : "splitk0");
  if (b && b->bytes > 0 && e->work.ws) {
    p.splitk_ws = reinterpret_cast<float*>(e->work.ws + b->off);
    p.splitk_ws_bytes = b->bytes;
  }
  if (lb) { p.m_split = m_split; p.W_b = lb->w; p.bias_b = lb->b; p.gate_b = gate_b; }
  HIP_TRY(mc::launch_linear_bf16(l, out, A, lda, M, p, epi, s));
  return MC_OK;
}

// ---- fp8_linear: where the quantised rows of a row range live ("aq" / "a_mx", layout at the top of the file)
// The range's region of "a_mx": the text range, the image range or the joint range of the single blocks.
struct MxRegion {
  uint8_t* base; long rows_pad;
};
MxRegion mx_region(const mc_mmdit* e, int row0, int rows) {
  const size_t Ltp = align_up(e->Lt, 256), Lip = align_up(e->Li, 256);
  const size_t blocks = (size_t)5 * e->d / 32 + (e->fp8 == 3 ? e->d / 32 : 0);   // per text / image row
  uint8_t* m = e->buf<uint8_t>("a_mx");
  if (row0 == e->txt0 && rows == e->Lt) return {m, (long)Ltp};
  if (row0 == e->img0 && rows == e->Li) return {m + blocks * Ltp, (long)Lip};
  return {m + blocks * (Ltp + Lip), (long)e->Sp};   // rows [0, S)
}
// columns [col0, ..) of "aq" rows [row0, row0 + rows) with their scales; o_proj: the scales of the rows an output projection
// of a double block reads (mode 3), behind the region's 5d/32 blocks
struct MxDst {
  uint8_t* q; long ld;
  uint8_t* mx; long rows_pad;
  MxRows rows() const { return {q, ld, mx, rows_pad}; }
};
MxDst mx_at(const mc_mmdit* e, int row0, int rows, int col0, bool o_proj = false) {
  const MxRegion r = mx_region(e, row0, rows);
  const size_t blk = o_proj ? (size_t)5 * e->d / 32 : (size_t)col0 / 32;
  const long ld = mc::mx_row_bytes(e->mx_fmt, 5L * e->d);   // col0 is a multiple of 32
  return {e->buf<uint8_t>("aq") + (size_t)row0 * ld + mc::mx_row_bytes(e->mx_fmt, col0), ld, r.base + blk * r.rows_pad, r.rows_pad};
}
// the fused-quantising GELU epilogue of the engine's format
int gelu_quant_epi(const mc_mmdit* e) { return mc::mx_info(e->mx_fmt).gelu_epi; }
// do the producers (the LayerNorm tail, MLP-in's GELU epilogue) write the quantised rows themselves?  e2m3 has no such producer
bool fused_quant(const mc_mmdit* e) { return mc::g_fp8_fused_quant && e->mx_fmt != mc::MX_E2M3; }
// bf16 rows -> their place in "aq" (the separate quantise pass: the attention output, and everything with fp8_fused_quant 0)
mc_status mx_quantise(const mc_mmdit* e, const bf16_t* rows_bf16, long ld, int rows, int K, const MxDst& to, hipStream_t s) {
  HIP_TRY(mc::launch_quantize_rows_mx(e->mx_fmt, rows_bf16, nullptr, ld, rows, K, to.q, to.ld, to.mx, to.rows_pad, s));
  return MC_OK;
}
// LayerNorm + modulate of "x" rows [row0, row0 + rows) as the operand of `l`: a bf16 Linear reads "xn"; an MX Linear reads
// "aq"[:, 0:d] (*a8), written by the LayerNorm kernel itself or, fp8_fused_quant 0, quantised from "xn" (the same bits)
mc_status ln_for_linear(const mc_mmdit* e, const Linear& l, int row0, int rows, const float* scale, const float* shift, MxRows* a8,
                        hipStream_t s) {
  const int d = e->d;
  const float* x = e->buf<float>("x") + (size_t)row0 * d;
  bf16_t* xn = e->buf<bf16_t>("xn") + (size_t)row0 * d;
  if (l.mx && fused_quant(e)) {
    const MxDst to = mx_at(e, row0, rows, 0);
    *a8 = to.rows();
    if (e->mx_fmt == mc::MX_E2M1) HIP_TRY(mc::launch_ln_modulate_mxfp4(x, d, scale, shift, 0, 1e-6f, to.q, to.ld, to.mx, to.rows_pad, rows, d, s));
    else HIP_TRY(mc::launch_ln_modulate_fp8(x, d, scale, shift, 0, 1e-6f, to.q, to.ld, nullptr, to.mx, to.rows_pad, rows, d, s));
    return MC_OK;
  }
  HIP_TRY(mc::launch_ln_modulate(x, d, nullptr, 0, scale, shift, 0, 1e-6f, xn, d, nullptr, 0, rows, d, s));
  if (l.mx) {
    const MxDst to = mx_at(e, row0, rows, 0);
    *a8 = to.rows();
    MC_TRY(mx_quantise(e, xn, d, rows, d, to, s));
  }
  return MC_OK;
}

// the gated residual epilogue on rows [row0, ..) of "x": x += gate * y, and with a capture destination (joint row index, the
// LAST block's output GEMM) the MagCache residual R = x_new - x0 as well.  Returns the epilogue to launch with.
int resid_epi(const mc_mmdit* e, mc::GemmParams& p, int row0, const float* gate, float* capture_to) {
  const size_t off = (size_t)row0 * e->d;
  p.X = e->buf<float>("x") + off; p.ldx = e->d; p.gate = gate;
  if (!capture_to) return mc::EPI_RESID_GATE;
  p.X0 = e->buf<bf16_t>("x0") + off; p.ldx0 = e->d;
  p.R = capture_to + off; p.ldr = e->d;
  return mc::EPI_RESID_CAPTURE;
}

// ---------------------------------------------------------------------------------------------- token geometry
// What a call may change (mc_mmdit_set_geometry): image tokens, the HunyuanVideo latent grid, the text length.  Everything
// below is a function of it and of what mc_mmdit_create fixed for good (family, widths, depths, the sequence-parallel
// shard) -- mc_mmdit_create and mc_mmdit_set_geometry share it.
struct Geometry {
  int img_tokens, latent_f, latent_h, latent_w, txt_len;
};
struct Rows {  // the derived integers of mc_mmdit
  int Li, Lt, S, Sp, Lrp, tok0, img0, txt0;
};

mc_status check_geometry(const mc_mmdit_config& c, const Geometry& g, int P, int rank) {
  if (g.txt_len <= 0) return fail(MC_EINVAL, "bad text geometry");
  if (g.img_tokens <= 0) return fail(MC_EINVAL, "img_tokens must be positive");
  if (c.family == MC_FAMILY_HUNYUAN &&
      (g.latent_f <= 0 || g.latent_h <= 0 || g.latent_w <= 0 || (g.latent_h & 1) || (g.latent_w & 1) ||
       g.img_tokens != g.latent_f * (g.latent_h / 2) * (g.latent_w / 2)))
    return fail(MC_EINVAL, "img_tokens must equal F*(H/2)*(W/2) of the latent grid");
  if (rank < 0 || rank >= P || (g.img_tokens % P) != 0)
    return fail(MC_EINVAL, "bad sequence-parallel geometry: rank %d of %d, %d image tokens", rank, P, g.img_tokens);
  return MC_OK;
}

Rows derive_rows(int family, const Geometry& g, int P, int rank) {
  const bool hy = family == MC_FAMILY_HUNYUAN;
  Rows r;
  r.Li = g.img_tokens / P; r.Lt = g.txt_len;
  r.tok0 = rank * r.Li;
  r.Lrp = (int)align_up(r.Li, 256);
  r.S = r.Li + r.Lt;
  r.Sp = (int)align_up(r.S, 256);
  r.img0 = hy ? 0 : r.Lt;
  r.txt0 = hy ? r.Li : 0;
  return r;
}

void apply_geometry(mc_mmdit* e, const Geometry& g, const Rows& r) {
  e->cfg.img_tokens = g.img_tokens; e->cfg.txt_len = g.txt_len;
  e->cfg.latent_f = g.latent_f; e->cfg.latent_h = g.latent_h; e->cfg.latent_w = g.latent_w;
  e->Li = r.Li; e->Lt = r.Lt; e->S = r.S; e->Sp = r.Sp; e->Lrp = r.Lrp;
  e->tok0 = r.tok0; e->img0 = r.img0; e->txt0 = r.txt0;
}

// the workspace of a geometry: needs of `e` only what mc_mmdit_create fixed (cfg widths, d, H, P, Kp, mod_rows)
void plan_workspace(const mc_mmdit* e, const Rows& r, mc::Workspace& ws) {
  const mc_mmdit_config& c = e->cfg;
  const bool qw = c.family == MC_FAMILY_QWEN;
  const size_t d = e->d, Sp = r.Sp, Li = r.Li;
  const size_t Ltp = align_up(r.Lt, 256);
  ws.add("x", Sp * d * 4);
  ws.add("x0", Sp * d * 2);
  ws.add("xn", Sp * d * 2);
  ws.add("qkv", (Sp + 64) * 3 * d * 2);        // + one key tile of slack behind the text rows
  if (e->P > 1) {
    ws.add("kv_gather", (size_t)e->P * r.Lrp * 2 * d * 2);   // image K|V of every rank
    ws.add("attn_lse", (size_t)e->H * Sp * 4);
  } else if (qw) {
    ws.add("attn_lse", (size_t)e->H * Sp * 4);                // image keys, then the valid text keys merged
  }
  ws.add("am", Sp * 5 * d * 2);               // also the fp32 [img, d] head operand after the last block
  ws.add("tokens", align_up(Li, 256) * e->Kp * 2);
  ws.add("txt_in", Ltp * c.txt_dim * 2);
  ws.add("txt_e", Ltp * d * 2);
  ws.add("emod", e->mod_rows * 4);
  ws.add("vecs", 16 * d * 4 + (size_t)c.txt_dim * 4 + 1024);   // sinusoids, hidden vectors, vec, c, gates
  ws.add("head_tokens", Li * 64 * 4);
  ws.add("residual0", Sp * d * 4);
  if (c.calibration) ws.add("residual1", Sp * d * 4);
  if (qw) {   // the uncond branch's slots (Qwen-Image only: the other families are guidance distilled, one branch)
    ws.add(c.calibration ? "residual2" : "residual1", Sp * d * 4);
    if (c.calibration) ws.add("residual3", Sp * d * 4);
  }
  {
    // split-K scratch (gemm_bf16_v2): the largest any GEMM of a block wants, one buffer per stream that may run GEMMs
    // (by shape: present at small geometries only, so the plan is not monotone in the token count)
    size_t need_all = 0, need_txt = 0;
    auto upd = [&](size_t& n, int M, int N, int K, int epi) { n = std::max(n, mc::gemm_splitk_ws_need(M, N, K, epi)); };
    for (int M : {(int)Li, r.Lt, r.S}) {
      for (size_t* n : {&need_all, M == r.Lt ? &need_txt : &need_all}) {
        upd(*n, M, 3 * d, d, mc::EPI_BF16);
        upd(*n, M, d, d, mc::EPI_RESID_GATE);
        upd(*n, M, 4 * d, d, mc::EPI_GELU_BF16);
        upd(*n, M, d, 4 * d, mc::EPI_RESID_GATE);
        upd(*n, M, d, 5 * d, mc::EPI_RESID_GATE);
      }
    }
    if (need_all) ws.add("splitk0", need_all);
    if (need_txt) ws.add("splitk1", need_txt);
  }
  ws.add("calib_partial", (2048 * 4 + 2) * 8);   // + the arrival ticket of calib_stats_kernel
  ws.add("calib_sums", 64);
  ws.add("calib_stats", 64);
  if (c.fp8_linear) {   // behind everything else: the plan of a bf16 engine does not change
    ws.add("aq", Sp * (size_t)mc::mx_row_bytes(e->mx_fmt, 5L * d));
    ws.add("a_mx", (5 * d / 32 + (c.fp8_linear == 3 ? d / 32 : 0)) * (Ltp + align_up(Li, 256)) + 5 * d / 32 * Sp);
  }
}

// (re)allocate the RoPE table for `rows` rows where it is shorter, and set every row to the identity rotation
mc_status rope_identity(mc_mmdit* e, int rows) {
  if (rows > e->cs_rows) {
    float* grown = nullptr;
    MC_TRY(e->weights.alloc(&grown, (size_t)rows * 128));
    if (e->cs) e->weights.release(e->cs);
    e->cs = grown;
    e->cs_rows = rows;
  }
  std::vector<float> ident((size_t)e->cs_rows * 128);
  for (size_t i = 0; i < ident.size(); i += 2) { ident[i] = 1.f; ident[i + 1] = 0.f; }
  if (hipMemcpy(e->cs, ident.data(), ident.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return fail(MC_EHIP, "RoPE table upload failed");
  return MC_OK;
}

// "ip_out" [rows, d] in the store, grown where it is shorter (never inside a forward)
mc_status ip_grow_out(mc_mmdit* e, int rows) {
  if (rows <= e->ip_out_rows) return MC_OK;
  bf16_t* grown = nullptr;
  MC_TRY(e->weights.alloc(&grown, (size_t)rows * e->d));
  if (e->ip_out) e->weights.release(e->ip_out);
  e->ip_out = grown;
  e->ip_out_rows = rows;
  return MC_OK;
}

// what a (re)bound or re-planned workspace means for the state: nothing cached, pad rows to be cleaned by the next forward
mc_status forget_workspace_state(mc_mmdit* e) {
  e->have_res[0] = e->have_res[1] = e->have_stats = e->pads_clean = false;
  if (e->work.ws) HIP_TRY(hipMemset(e->buf<double>("calib_partial") + 2048 * 4, 0, 16));   // arrival ticket of calib_stats_kernel
  return MC_OK;
}

}  // namespace

extern "C" {

// mc_mmdit_config only ever grows at its END, and a zero in a new field keeps the behaviour older callers had: a caller built
// against an older header passes ITS sizeof(mc_mmdit_config) and the tail reads as zeros.  mc_mmdit_create is the entry
// point of the first layout (up to sp_size) and reads no further.
static mc_status create_engine(const mc_mmdit_config& c, mc_mmdit** out);

mc_status mc_mmdit_create_sized(const mc_mmdit_config* cfg, size_t cfg_bytes, mc_mmdit** out) {
  if (!cfg || !out) return fail(MC_EINVAL, "null argument");
  if (cfg_bytes < offsetof(mc_mmdit_config, fp8_linear) || cfg_bytes > sizeof(mc_mmdit_config) || (cfg_bytes % sizeof(int)) != 0)
    return fail(MC_EINVAL, "mc_mmdit_config of %zu bytes: this library knows %zu (first layout) .. %zu", cfg_bytes,
                offsetof(mc_mmdit_config, fp8_linear), sizeof(mc_mmdit_config));
  mc_mmdit_config full;
  memset(&full, 0, sizeof(full));
  memcpy(&full, cfg, cfg_bytes);
  return create_engine(full, out);
}

mc_status mc_mmdit_create(const mc_mmdit_config* cfg, mc_mmdit** out) {
  return mc_mmdit_create_sized(cfg, offsetof(mc_mmdit_config, fp8_linear), out);
}

static mc_status create_engine(const mc_mmdit_config& c, mc_mmdit** out) {
  const bool hy = c.family == MC_FAMILY_HUNYUAN;
  const bool qw = c.family == MC_FAMILY_QWEN;
  if (c.family != MC_FAMILY_FLUX && !hy && !qw) return fail(MC_EINVAL, "unknown family %d", c.family);
  if (c.num_heads <= 0 || c.dim != c.num_heads * 128) return fail(MC_EINVAL, "dim must be num_heads * 128 (head_dim 128)");
  // options "mx_fp4" / "mx_fp6" (latched here, as mc_create latches them): the element format of the MX copies.  The MX GEMMs
  // tile K by 256 from 512 up; every such Linear reads dim, 4 dim or 5 dim features, so the first one decides -- refused by name
  mc::MxFormat mx_fmt;
  MC_TRY(mc::latch_mx_format(c.fp8_linear == 2 || c.fp8_linear == 3, &mx_fmt));
  if (mx_fmt != mc::MX_E4M3)
    MC_TRY(mc::check_mx_k(mx_fmt, "q|k|v / MLP-in (in_features = dim; MLP-out reads 4 dim, a single block's linear2 5 dim)", c.dim));
  if ((c.dim % 256) != 0) return fail(MC_EINVAL, "dim %d must be a multiple of 256", c.dim);
  if (c.n_double < 0 || c.n_single < 0 || c.n_double + c.n_single == 0) return fail(MC_EINVAL, "no blocks");
  if (c.txt_dim <= 0 || (c.txt_dim % 64) != 0 || (!qw && (c.vec_dim <= 0 || (c.vec_dim % 8) != 0)))
    return fail(MC_EINVAL, "bad text geometry");
  if (qw) {
    if (c.n_single != 0) return fail(MC_EINVAL, "Qwen-Image has no single-stream blocks (n_single %d)", c.n_single);
    if (c.vec_dim != 0) return fail(MC_EINVAL, "Qwen-Image has no pooled text vector (vec_dim %d)", c.vec_dim);
    if (c.sp_size > 1) return fail(MC_EINVAL, "Qwen-Image runs on one GPU (sp_size %d)", c.sp_size);
  }
  if (hy) {
    if (c.out_channels * 4 > 64) return fail(MC_EINVAL, "out_channels*4 > 64 unsupported by the head kernel");
  } else if (c.out_channels > 64 || c.refiner_depth != 0) {
    return fail(MC_EINVAL, "FLUX / Qwen-Image: out_channels <= 64, no refiner");
  }
  const Geometry geo = {c.img_tokens, c.latent_f, c.latent_h, c.latent_w, c.txt_len};
  const int P = c.sp_size > 0 ? c.sp_size : 1;
  MC_TRY(check_geometry(c, geo, P, c.sp_rank));
  if (c.fp8_linear != 0 && c.fp8_linear != 2 && c.fp8_linear != 3)
    return fail(MC_EINVAL, "fp8_linear must be 0, 2 (MX block scales: q|k|v, MLP-in, MLP-out, the single block's linear1) or 3 "
                           "(MX, the output projections too); 1 (per-row scales) has no MM-DiT path");
  if (c.fp8_linear && c.dim < 512) return fail(MC_EINVAL, "fp8_linear needs dim >= 512 (dim %d)", c.dim);
  if (c.fp8_linear && P > 1) return fail(MC_EINVAL, "fp8_linear runs on one GPU (sp_size %d)", P);
  std::unique_ptr<mc_mmdit, void (*)(mc_mmdit*)> own(new mc_mmdit(), mc_mmdit_destroy);   // every early return frees it
  mc_mmdit* e = own.get();
  e->cfg = c;
  e->fp8 = c.fp8_linear;
  e->mx_fmt = mx_fmt;
  e->P = P;
  e->rank = c.sp_rank;
  e->d = c.dim; e->H = c.num_heads;
  const Rows rows = derive_rows(c.family, geo, P, c.sp_rank);
  apply_geometry(e, geo, rows);
  e->Kin = hy ? c.in_channels * 4 : c.in_channels;
  e->Kp = (int)align_up(e->Kin, 64);
  e->out_feat = hy ? c.out_channels * 4 : c.out_channels;
  const size_t d = e->d;
  const bool flux = c.family == MC_FAMILY_FLUX;
  mc::WeightStore& W = e->weights;
  // fp8_linear only decides which Linears keep an e4m3 copy with MX block scales: 2 = those that read a LayerNorm or GELU
  // output, 3 = those that read the attention output too.  The embedders, the modulation matrix, the token refiner and the
  // head stay bf16.
  const mc::Quant q_big = c.fp8_linear >= 2 ? mc::QUANT_MX : mc::QUANT_NONE;
  const mc::Quant q_out = c.fp8_linear == 3 ? mc::QUANT_MX : mc::QUANT_NONE;
  auto vec128 = [&](float*& v, const std::string& name) { return W.add_f32(v, name, 128); };   // a per-head norm weight
  auto mlp2 = [&](Mlp2& m, size_t k_in, const std::string& l1, const std::string& l2) {
    MC_TRY(W.add_linear(m.l1, l1, {{"", d}}, k_in));
    return W.add_linear(m.l2, l2, {{"", d}}, d);
  };

  // ---- embeds
  // Qwen-Image slots: diffusers models/transformers/transformer_qwenimage.py (QwenImageTransformer2DModel: img_in,
  // txt_norm, txt_in, time_text_embed.timestep_embedder, transformer_blocks.{i}.{img_mod.1, txt_mod.1, attn.*,
  // img_mlp.net.{0.proj,2}, txt_mlp.net.{0.proj,2}}, norm_out.linear, proj_out)
  MC_TRY(W.alloc_linear(e->img_in, d, e->Kp));
  HIP_TRY(hipMemset(e->img_in.w, 0, d * e->Kp * 2));
  mc::Slot& w_in = W.add_parts(e->img_in, "", {{flux ? "x_embedder" : qw ? "img_in" : "img_in.proj", d}});
  if (e->Kin != e->Kp) {   // given [d, Kin], stored [d, Kp]: Kin padded to a GEMM K step
    w_in.numel = d * e->Kin;
    w_in.pad = {d, (size_t)e->Kin, (size_t)e->Kp};
  }
  MC_TRY(W.add_linear(e->txt_in, "", {{flux ? "context_embedder" : qw ? "txt_in" : "txt_in.input_embedder", d}}, c.txt_dim));
  if (qw) {
    MC_TRY(W.add_f32(e->w_txt_norm, "txt_norm.weight", c.txt_dim));
    MC_TRY(mlp2(e->time_mlp, 256, "time_text_embed.timestep_embedder.linear_1", "time_text_embed.timestep_embedder.linear_2"));
  } else if (flux) {
    MC_TRY(mlp2(e->time_mlp, 256, "time_text_embed.timestep_embedder.linear_1", "time_text_embed.timestep_embedder.linear_2"));
    MC_TRY(mlp2(e->guid_mlp, 256, "time_text_embed.guidance_embedder.linear_1", "time_text_embed.guidance_embedder.linear_2"));
    MC_TRY(mlp2(e->vec_mlp, c.vec_dim, "time_text_embed.text_embedder.linear_1", "time_text_embed.text_embedder.linear_2"));
  } else {
    MC_TRY(mlp2(e->time_mlp, 256, "time_in.mlp.0", "time_in.mlp.2"));
    MC_TRY(mlp2(e->guid_mlp, 256, "guidance_in.mlp.0", "guidance_in.mlp.2"));
    MC_TRY(mlp2(e->vec_mlp, c.vec_dim, "vector_in.in_layer", "vector_in.out_layer"));
    MC_TRY(mlp2(e->ref_t_mlp, 256, "txt_in.t_embedder.mlp.0", "txt_in.t_embedder.mlp.2"));
    MC_TRY(mlp2(e->ref_c_mlp, c.txt_dim, "txt_in.c_embedder.linear_1", "txt_in.c_embedder.linear_2"));
    e->refiners.resize(c.refiner_depth);
    for (int i = 0; i < c.refiner_depth; ++i) {
      Refiner& r = e->refiners[i];
      const std::string p = "txt_in.individual_token_refiner.blocks." + std::to_string(i) + ".";
      MC_TRY(W.add_linear(r.qkv, p, {{"self_attn_qkv", 3 * d}}, d));
      MC_TRY(W.add_linear(r.o, p, {{"self_attn_proj", d}}, d));
      MC_TRY(W.add_linear(r.fc1, p, {{"mlp.fc1", 4 * d}}, d));
      MC_TRY(W.add_linear(r.fc2, p, {{"mlp.fc2", d}}, 4 * d));
      MC_TRY(W.add_linear(r.ada, p, {{"adaLN_modulation.1", 2 * d}}, d));
      float** norms[4] = {&r.n1w, &r.n1b, &r.n2w, &r.n2b};
      const char* names[4] = {"norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"};
      for (int k = 0; k < 4; ++k) MC_TRY(W.add_f32(*norms[k], p + names[k], d));
    }
  }
  // ---- fused modulation matrix: every block's AdaLN linear stacked, one GEMV per forward; the blocks add their parts
  e->mod_rows = e->mod_final() + 2 * d;
  MC_TRY(W.alloc_linear(e->mod, e->mod_rows, d));
  // ---- blocks
  e->dimg.resize(c.n_double); e->dtxt.resize(c.n_double);
  for (int i = 0; i < c.n_double; ++i) {
    const std::string p = (hy ? "double_blocks." : "transformer_blocks.") + std::to_string(i) + ".";
    for (int k = 0; k < 2; ++k) {   // image stream, text stream
      Stream& t = k ? e->dtxt[i] : e->dimg[i];
      if (hy) {
        const std::string q = p + (k ? "txt" : "img");
        W.add_parts(e->mod, q, {{"_mod.linear", 6 * d}}, e->mod_double(i, k));
        MC_TRY(W.add_linear(t.qkv, q, {{"_attn_qkv", 3 * d}}, d, q_big, mx_fmt));
        MC_TRY(W.add_linear(t.o, q, {{"_attn_proj", d}}, d, q_out, mx_fmt));
        MC_TRY(W.add_linear(t.fc1, q, {{"_mlp.fc1", 4 * d}}, d, q_big, mx_fmt));
        MC_TRY(W.add_linear(t.fc2, q, {{"_mlp.fc2", d}}, 4 * d, q_big, mx_fmt));
        MC_TRY(vec128(t.qn, q + "_attn_q_norm.weight"));
        MC_TRY(vec128(t.kn, q + "_attn_k_norm.weight"));
      } else {
        // modulation chunk order shift, scale, gate (attention), shift, scale, gate (MLP) in both families
        const std::string ff = qw ? (k ? "txt_mlp" : "img_mlp") : (k ? "ff_context" : "ff");
        W.add_parts(e->mod, p, {{qw ? (k ? "txt_mod.1" : "img_mod.1") : (k ? "norm1_context.linear" : "norm1.linear"), 6 * d}},
                    e->mod_double(i, k));
        if (k) MC_TRY(W.add_linear(t.qkv, p, {{"attn.add_q_proj", d}, {"attn.add_k_proj", d}, {"attn.add_v_proj", d}}, d, q_big, mx_fmt));
        else MC_TRY(W.add_linear(t.qkv, p, {{"attn.to_q", d}, {"attn.to_k", d}, {"attn.to_v", d}}, d, q_big, mx_fmt));
        MC_TRY(W.add_linear(t.o, p, {{k ? "attn.to_add_out" : "attn.to_out.0", d}}, d, q_out, mx_fmt));
        MC_TRY(W.add_linear(t.fc1, p, {{ff + ".net.0.proj", 4 * d}}, d, q_big, mx_fmt));
        MC_TRY(W.add_linear(t.fc2, p, {{ff + ".net.2", d}}, 4 * d, q_big, mx_fmt));
        MC_TRY(vec128(t.qn, p + (k ? "attn.norm_added_q.weight" : "attn.norm_q.weight")));
        MC_TRY(vec128(t.kn, p + (k ? "attn.norm_added_k.weight" : "attn.norm_k.weight")));
      }
    }
  }
  e->singles.resize(c.n_single);
  for (int i = 0; i < c.n_single; ++i) {
    Single& g = e->singles[i];
    const std::string p = (flux ? "single_transformer_blocks." : "single_blocks.") + std::to_string(i) + ".";
    W.add_parts(e->mod, p, {{flux ? "norm.linear" : "modulation.linear", 3 * d}}, e->mod_single(i));
    if (flux) {
      MC_TRY(W.add_linear(g.in, p, {{"attn.to_q", d}, {"attn.to_k", d}, {"attn.to_v", d}, {"proj_mlp", 4 * d}}, d, q_big, mx_fmt));
      MC_TRY(W.add_linear(g.out, p, {{"proj_out", d}}, 5 * d, q_out, mx_fmt));
    } else {
      MC_TRY(W.add_linear(g.in, p, {{"linear1", 7 * d}}, d, q_big, mx_fmt));
      MC_TRY(W.add_linear(g.out, p, {{"linear2", d}}, 5 * d, q_out, mx_fmt));
    }
    MC_TRY(vec128(g.qn, p + (flux ? "attn.norm_q.weight" : "q_norm.weight")));
    MC_TRY(vec128(g.kn, p + (flux ? "attn.norm_k.weight" : "k_norm.weight")));
  }
  // ---- final layer
  // (Qwen-Image's head is FLUX's: AdaLayerNormContinuous, chunk order scale, shift)
  W.add_parts(e->mod, "", {{!hy ? "norm_out.linear" : "final_layer.adaLN_modulation.1", 2 * d}}, e->mod_final());
  const std::string head = !hy ? "proj_out." : "final_layer.linear.";
  MC_TRY(W.add_f32(e->w_head, head + "weight", (size_t)e->out_feat * d));
  MC_TRY(W.add_f32(e->b_head, head + "bias", e->out_feat));
  // upstream (c, pt, ph, pw) channel-major; launch_unpatchify wants (ph, pw, c)
  if (hy) W.slots.at(head + "weight").perm_c = W.slots.at(head + "bias").perm_c = c.out_channels;
  // ---- RoPE table, identity rotation until mc_mmdit_set_rope
  MC_TRY(rope_identity(e, e->Sp));
  // ---- workspace plan
  plan_workspace(e, rows, e->work);
  // side stream and fork / join events of the (optional) two-stream double block: created here, never inside a forward
  // (a forward may run under stream capture)
  HIP_TRY(hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking));
  for (int i = 0; i < 8; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&e->ev_fork[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_join[i], hipEventDisableTiming));
  }
  *out = own.release();
  return MC_OK;
}

void mc_mmdit_destroy(mc_mmdit* e) {
  if (!e) return;
  if (e->side) (void)hipStreamDestroy(e->side);
  for (int i = 0; i < 8; ++i) {   // a create that failed midway made only some of them
    if (e->ev_fork[i]) (void)hipEventDestroy(e->ev_fork[i]);
    if (e->ev_join[i]) (void)hipEventDestroy(e->ev_join[i]);
  }
  e->weights.free_all();
  delete e;
}

size_t mc_mmdit_workspace_bytes(const mc_mmdit* e) { return e ? e->work.need : 0; }

int mc_mmdit_mx_fp4(const mc_mmdit* e) { return e && e->mx_fmt == mc::MX_E2M1 ? 1 : 0; }
int mc_mmdit_mx_fp6(const mc_mmdit* e) { return e && e->mx_fmt == mc::MX_E2M3 ? 1 : 0; }

mc_status mc_mmdit_set_workspace(mc_mmdit* e, void* ws_dev, size_t bytes) {
  if (!e) return fail(MC_EINVAL, "null argument");
  MC_TRY(e->work.bind(ws_dev, bytes));
  return forget_workspace_state(e);
}

mc_status mc_mmdit_geometry_bytes(const mc_mmdit* e, int img_tokens, int latent_f, int latent_h, int latent_w, int txt_len,
                                  size_t* bytes) {
  if (!e || !bytes) return fail(MC_EINVAL, "null argument");
  const Geometry g = {img_tokens, latent_f, latent_h, latent_w, txt_len};
  MC_TRY(check_geometry(e->cfg, g, e->P, e->rank));
  mc::Workspace plan;
  plan_workspace(e, derive_rows(e->cfg.family, g, e->P, e->rank), plan);
  *bytes = plan.need;
  return MC_OK;
}

mc_status mc_mmdit_set_geometry(mc_mmdit* e, int img_tokens, int latent_f, int latent_h, int latent_w, int txt_len) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->begun) return fail(MC_ESTATE, "mc_mmdit_set_geometry between mc_mmdit_begin and mc_mmdit_end");
  if (e->P > 1)
    return fail(MC_EINVAL, "mc_mmdit_set_geometry: a sequence-parallel engine (sp_size %d) keeps the geometry it was created with", e->P);
  const Geometry g = {img_tokens, latent_f, latent_h, latent_w, txt_len};
  MC_TRY(check_geometry(e->cfg, g, e->P, e->rank));
  const Rows r = derive_rows(e->cfg.family, g, e->P, e->rank);
  mc::Workspace plan;
  plan_workspace(e, r, plan);
  if (e->work.ws && plan.need > e->work.bound)
    return fail(MC_EINVAL, "geometry needs a workspace of %zu bytes, %zu bytes are bound (mc_mmdit_set_workspace)", plan.need,
                e->work.bound);
  // earlier forwards may still be reading the RoPE table and the buffers of the old plan
  HIP_TRY(hipDeviceSynchronize());
  MC_TRY(rope_identity(e, r.Sp));   // the steps that can fail for lack of memory: before anything changes
  if (!e->ip.empty()) MC_TRY(ip_grow_out(e, r.Li));
  MC_TRY(e->work.replan(plan));
  apply_geometry(e, g, r);
  e->cn_double.clear();   // the samples were [img_tokens, d] of the old geometry
  e->cn_single.clear();
  return forget_workspace_state(e);
}

mc_status mc_mmdit_buffer_info(const mc_mmdit* e, const char* name, size_t* offset, size_t* bytes) {
  if (!e || !name) return fail(MC_EINVAL, "null argument");
  std::string n(name);
  // "residual": the image rows of the slot that holds the cache of the last forward's branch; "residual_b<k>": branch k's
  const bool res = (n == "residual" || n == "residual_b0" || n == "residual_b1");
  if (res) {
    const int b = n == "residual" ? e->branch : n[10] - '0';
    if (b == 1 && e->cfg.family != MC_FAMILY_QWEN) return fail(MC_EINVAL, "unknown buffer '%s'", name);
    n = "residual" + std::to_string(e->res_index(b, e->res_cur[b]));
  }
  MC_TRY(e->work.info(n, offset, bytes));
  if (res && offset) *offset += (size_t)e->img0 * e->d * 4;
  if (res && bytes) *bytes = (size_t)e->Li * e->d * 4;
  return MC_OK;
}

mc_status mc_mmdit_set_weight(mc_mmdit* e, const char* name, const void* src_dev, mc_dtype dtype, const int64_t* shape,
                              int ndim, mc_stream stream) {
  if (!e || !name || !src_dev || !shape) return fail(MC_EINVAL, "null argument");
  return e->weights.set(name, src_dev, dtype, shape, ndim, (hipStream_t)stream);
}

int mc_mmdit_weights_missing(const mc_mmdit* e, char* buf, size_t buflen) {
  return e ? e->weights.missing(buf, buflen) : -1;
}

// ---- LoRA adapters: the store does the work (host.h), between forwards only
static mc_status lora_entry(const mc_mmdit* e, const char* what) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->begun) return fail(MC_ESTATE, "%s between mc_mmdit_begin and mc_mmdit_end", what);
  return MC_OK;
}

mc_status mc_mmdit_lora_set(mc_mmdit* e, const char* adapter, const char* weight_name, const void* down_dev,
                            const int64_t* down_shape, const void* up_dev, const int64_t* up_shape, mc_dtype dtype, float factor,
                            mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_mmdit_lora_set"));
  return e->weights.lora_set(adapter, weight_name, down_dev, down_shape, up_dev, up_shape, dtype, factor, (hipStream_t)stream);
}

mc_status mc_mmdit_lora_set_kron(mc_mmdit* e, const char* adapter, const char* weight_name, const void* w1_dev,
                                 const int64_t* w1_shape, const void* w2_dev, const int64_t* w2_shape, mc_dtype dtype, float factor,
                                 mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_mmdit_lora_set_kron"));
  return e->weights.lora_set_kron(adapter, weight_name, w1_dev, w1_shape, w2_dev, w2_shape, dtype, factor, (hipStream_t)stream);
}

mc_status mc_mmdit_lora_set_hada(mc_mmdit* e, const char* adapter, const char* weight_name, const void* u1_dev,
                                 const int64_t* u_shape, const void* d1_dev, const int64_t* d_shape, const void* u2_dev,
                                 const void* d2_dev, mc_dtype dtype, float factor, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_mmdit_lora_set_hada"));
  return e->weights.lora_set_hada(adapter, weight_name, u1_dev, u_shape, d1_dev, d_shape, u2_dev, d2_dev, dtype, factor,
                                  (hipStream_t)stream);
}

mc_status mc_mmdit_lora_set_magnitude(mc_mmdit* e, const char* adapter, const char* weight_name, const void* magnitude_dev,
                                      size_t numel, mc_dtype dtype, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_mmdit_lora_set_magnitude"));
  return e->weights.lora_set_magnitude(adapter, weight_name, magnitude_dev, numel, dtype, (hipStream_t)stream);
}

mc_status mc_mmdit_lora_scale(mc_mmdit* e, const char* adapter, float scale) {
  MC_TRY(lora_entry(e, "mc_mmdit_lora_scale"));
  return e->weights.lora_scale(adapter, scale);
}

mc_status mc_mmdit_lora_remove(mc_mmdit* e, const char* adapter) {
  MC_TRY(lora_entry(e, "mc_mmdit_lora_remove"));
  return e->weights.lora_remove(adapter);
}

mc_status mc_mmdit_lora_apply(mc_mmdit* e, mc_stream stream) {
  MC_TRY(lora_entry(e, "mc_mmdit_lora_apply"));
  return e->weights.lora_apply((hipStream_t)stream);
}

mc_status mc_mmdit_lora_info(const mc_mmdit* e, int* adapters, int* linears, size_t* base_bytes) {
  if (!e) return fail(MC_EINVAL, "null engine");
  e->weights.lora_info(adapters, linears, base_bytes);
  return MC_OK;
}

mc_status mc_mmdit_set_rope(mc_mmdit* e, const float* cos_dev, const float* sin_dev, int n_rows, mc_stream stream) {
  if (!e || !cos_dev || !sin_dev) return fail(MC_EINVAL, "null argument");
  const bool hy = e->cfg.family == MC_FAMILY_HUNYUAN;
  const int want = hy ? e->cfg.img_tokens : e->Lt + e->cfg.img_tokens;   // the table of the FULL sequence
  if (n_rows != want) return fail(MC_EINVAL, "RoPE table has %d rows, %d expected", n_rows, want);
  hipStream_t s = (hipStream_t)stream;
  // image rows of this rank's shard (global token positions), then -- FLUX -- the text rows
  const size_t img_src = (size_t)(hy ? 0 : e->Lt) + e->tok0;
  HIP_TRY(mc::launch_rope_table_from_cos_sin(cos_dev + img_src * 128, sin_dev + img_src * 128, 128, e->Li,
                                             e->cs + (size_t)e->img0 * 128, s));
  if (!hy) HIP_TRY(mc::launch_rope_table_from_cos_sin(cos_dev, sin_dev, 128, e->Lt, e->cs + (size_t)e->txt0 * 128, s));
  return MC_OK;
}

mc_status mc_mmdit_state_reset(mc_mmdit* e) {
  if (!e) return fail(MC_EINVAL, "null engine");
  e->have_res[0] = e->have_res[1] = e->have_stats = false;
  return MC_OK;
}

mc_status mc_mmdit_calib_stats(mc_mmdit* e, float out[3], mc_stream stream) {
  if (!e || !out) return fail(MC_EINVAL, "null argument");
  if (!e->have_stats) return fail(MC_ESTATE, "no calibration statistics: needs two MC_MODE_CALIB forwards");
  HIP_TRY(hipMemcpyAsync(out, e->buf<float>("calib_stats"), 12, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return MC_OK;
}

}  // extern "C"

namespace {

// y = W2 silu(W1 x + b1) + b2   (TimestepEmbedding / MLPEmbedder / TextProjection); h: scratch [d]
mc_status run_mlp2(const Mlp2& m, const float* x, float* h, float* y, int accumulate, hipStream_t s) {
  HIP_TRY(mc::launch_gemv_bf16w(m.l1.w, x, m.l1.b, h, m.l1.n_out, m.l1.k_in, 0, 0, 0, s));
  HIP_TRY(mc::launch_gemv_bf16w(m.l2.w, h, m.l2.b, y, m.l2.n_out, m.l2.k_in, 1, 0, accumulate, s));
  return MC_OK;
}

// ---------------------------------------------------------------------------------------------- attention
// The key sets (mc::Keys) of this engine; the rows between `valid` and `rows` are padded text rows, the neighbouring stream's
// rows or the zeroed tail of "qkv".
Keys local_keys(const mc_mmdit* e, int row0, int rows_pad, int valid) {   // rows [row0, ..) of the local "qkv"
  const bf16_t* k = e->buf<bf16_t>("qkv") + (size_t)row0 * 3 * e->d + e->d;
  return {k, k + e->d, 3L * e->d, 0, rows_pad, valid, 1, 0};
}
Keys image_keys(const mc_mmdit* e) { return local_keys(e, e->img0, (int)align_up(e->Li, 64), e->Li); }
Keys text_keys(const mc_mmdit* e) { return local_keys(e, e->txt0, (int)align_up(e->Lt, 64), e->txt_valid); }
// the image K|V shards of every rank in "kv_gather"; skip_shard_p1 = k + 1 leaves shard k out
Keys gathered_keys(const mc_mmdit* e, int skip_shard_p1) {
  const bf16_t* k = e->buf<bf16_t>("kv_gather");
  return {k, k + e->d, 2L * e->d, (long)e->Lrp * 2 * e->d, e->Lrp, e->Li, e->P, skip_shard_p1};
}

// rows [0, q_rows_pad) of "qkv" as queries over one key set -> "am"[:, 0:d].  lse_out: keep the log-sum-exp of this launch;
// lse_in: "am" already holds the result over other keys with that log-sum-exp, merge with it.
mc_status attend(const mc_mmdit* e, int q_rows_pad, const Keys& keys, const float* lse_in, float* lse_out, hipStream_t s) {
  HIP_TRY(mc::launch_attention_keys(e->buf<bf16_t>("qkv"), 3L * e->d, e->buf<bf16_t>("am"), 5L * e->d, q_rows_pad, e->H, keys,
                                    lse_in, lse_out, s));
  return MC_OK;
}

// HunyuanVideo txt_in = SingleTokenRefiner(text_states, t, mask)  (reference :75; upstream token_refiner.py):
// result in the text rows of x.  Works on rows [0, Ltp) of xn / qkv / am, which the main blocks overwrite later.
mc_status run_refiner(mc_mmdit* e, const float* txt_dev, int txt_valid, float* vecs, hipStream_t s) {
  const mc_mmdit_config& c = e->cfg;
  const int d = e->d, Lt = e->Lt;
  const int Ltp = (int)align_up(Lt, 256);
  float* sin_t = vecs;              // [256] sinusoid of t (written by the caller)
  float* hid = vecs + 2 * d;        // hidden scratch [d]
  float* cvec = vecs + 4 * d;       // c = t_embedder(t) + c_embedder(mean of the valid text states)
  float* gates = vecs + 5 * d;      // [2d]
  float* cmean = vecs + 16 * d;     // [txt_dim]
  MC_TRY(run_mlp2(e->ref_t_mlp, sin_t, hid, cvec, 0, s));
  HIP_TRY(mc::launch_colmean(txt_dev, c.txt_dim, txt_valid, c.txt_dim, cmean, s));
  MC_TRY(run_mlp2(e->ref_c_mlp, cmean, hid, cvec, 1, s));
  float* xt = e->buf<float>("x") + (size_t)e->txt0 * d;
  bf16_t* xn = e->buf<bf16_t>("xn");
  bf16_t* am = e->buf<bf16_t>("am");
  for (const Refiner& r : e->refiners) {
    HIP_TRY(mc::launch_gemv_bf16w(r.ada.w, cvec, r.ada.b, gates, 2 * d, d, 1, 0, 0, s));
    HIP_TRY(mc::launch_ln_modulate(xt, d, nullptr, 0, r.n1w, r.n1b, 1, 1e-6f, xn, d, nullptr, 0, Lt, d, s));
    mc::GemmParams p = {}, o = {}, f1 = {}, f2 = {};
    p.Cb = e->buf<bf16_t>("qkv"); p.ldc = 3 * d;
    MC_TRY(linear(e, r.qkv, Lt, xn, d, p, mc::EPI_BF16, s));
    MC_TRY(attend(e, Ltp, local_keys(e, 0, Ltp, txt_valid), nullptr, nullptr, s));
    const int epi_o = resid_epi(e, o, e->txt0, gates, nullptr);
    MC_TRY(linear(e, r.o, Lt, am, 5 * d, o, epi_o, s));
    HIP_TRY(mc::launch_ln_modulate(xt, d, nullptr, 0, r.n2w, r.n2b, 1, 1e-6f, xn, d, nullptr, 0, Lt, d, s));
    f1.Cb = am + d; f1.ldc = 5 * d;
    MC_TRY(linear(e, r.fc1, Lt, xn, d, f1, mc::EPI_SILU_BF16, s));
    const int epi_f2 = resid_epi(e, f2, e->txt0, gates + d, nullptr);
    MC_TRY(linear(e, r.fc2, Lt, am + d, 5 * d, f2, epi_f2, s));
  }
  return MC_OK;
}

// ---------------------------------------------------------------------------------------------- double block
// A double block runs over n = 1 or 2 row ranges of the joint buffers, each with its stream's weights and modulation vector:
// one stream per call (the two-stream modes; sequence parallel), or BOTH streams in merged launches (round 5, the default).
// The streams' Linears have the same shapes, so with two adjacent ranges the q|k|v, the output projection and MLP-out are
// one row-split GEMM each: with the range boundary on a 256-row tile boundary (FLUX: [text 512 ; image]) ONE launch
// (GemmParams.m_split: 216 / 72 / 72 x 3 tiles at 512^2 instead of 144 + 72 / 48 + 24 / 48 x 4 + 24 x 6 in two launches);
// HunyuanVideo's boundary (118 800 image rows first) is not on a tile boundary: launch_gemm_bf16 then runs the two launches.
// LayerNorm (per-stream modulation), head norm (per-stream weights) and MLP-in (192 + 96 tiles separately beat 288 together:
// two trips of 256 CUs) stay per range.
struct Range {
  const Stream* w;
  const float* mod;   // shift, scale, gate (attention), shift, scale, gate (MLP)
  int row0, rows;
};
bool double_block_merged(const mc_mmdit* e) {
  return g_mmdit_two_streams == 0 && e->P == 1 && e->Lt > 0 && e->Li > 0 && !e->fp8;
}

// the two streams of block `blk` as adjacent ranges in row order; img / txt: which of them is which
struct TwoStreams {
  Range r[2];
  int img, txt;
};
TwoStreams two_streams(const mc_mmdit* e, int blk, const float* emod) {
  TwoStreams t;
  t.txt = e->txt0 < e->img0 ? 0 : 1;
  t.img = 1 - t.txt;
  t.r[t.img] = {&e->dimg[blk], emod + e->mod_double(blk, 0), e->img0, e->Li};
  t.r[t.txt] = {&e->dtxt[blk], emod + e->mod_double(blk, 1), e->txt0, e->Lt};
  return t;
}

// one Linear of the block over all n ranges: rows from r[0].row0 on, row-split at the range boundary when n = 2
// (a8: the quantised rows of r[0] when the Linear is MX -- an fp8 engine runs a block one range at a time, n = 1)
mc_status range_linear(const mc_mmdit* e, const Range* r, int n, Linear Stream::*l, const bf16_t* A, long lda, const mc::GemmParams& p,
                       int epi, const float* gate_b, hipStream_t s, const MxRows* a8 = nullptr) {
  const int rows = r[0].rows + (n == 2 ? r[1].rows : 0);
  return linear(e, r[0].w->*l, rows, A, lda, p, epi, s, n == 2 ? &(r[1].w->*l) : nullptr, r[0].rows, gate_b, a8);
}

// ---- IP-Adapter: the adapters that count in double block `blk` (an image in the selected slot, a scale that is not 0)
int ip_live(const mc_mmdit* e, int blk, mc::IpKeys* keys) {
  int n = 0;
  if (e->ip_slot < 0 || blk >= e->cfg.n_double) return 0;
  for (const auto& a : e->ip) {
    const int k = a->keys[e->ip_slot];
    if (k <= 0 || a->scale[blk] == 0.f) continue;
    if (keys) keys[n] = {a->cache[e->ip_slot] + (size_t)blk * a->rows[e->ip_slot] * 2 * e->d, 2L * e->d, k, a->scale[blk]};
    ++n;
  }
  return n;
}
// "ip_out" = sum_j scale_j softmax(q_n K_j^T / sqrt(128)) V_j over the image rows, from the RAW q of "qkv"
mc_status ip_attend(const mc_mmdit* e, int blk, hipStream_t s) {
  mc::IpKeys keys[mc::kIpMaxAdapters];
  const int n = ip_live(e, blk, keys);
  if (n == 0) return MC_OK;
  HIP_TRY(mc::launch_ip_attention(e->buf<bf16_t>("qkv") + (size_t)e->img0 * 3 * e->d, 3L * e->d, e->dimg[blk].qn, 1e-6f, keys, n,
                                  e->ip_out, e->d, e->Li, e->H, s));
  return MC_OK;
}

// before the joint attention: LN + modulate, QKV, per-head q/k norm, RoPE
// phases (diagnostic split, tests/two_stream_bisect.py): 1 = LN + QKV GEMM, 2 = head norm + RoPE, 3 = both
mc_status double_pre(const mc_mmdit* e, const Range* r, int n, hipStream_t s, int phases = 3) {
  const int d = e->d;
  bf16_t* xn = e->buf<bf16_t>("xn");
  bf16_t* qkv = e->buf<bf16_t>("qkv");
  if (phases & 1) {
    MxRows a8 = {};
    for (int i = 0; i < n; ++i)
      MC_TRY(ln_for_linear(e, r[i].w->qkv, r[i].row0, r[i].rows, r[i].mod + d, r[i].mod, &a8, s));
    mc::GemmParams p = {};
    p.Cb = qkv + (size_t)r[0].row0 * 3 * d; p.ldc = 3 * d;
    MC_TRY(range_linear(e, r, n, &Stream::qkv, xn + (size_t)r[0].row0 * d, d, p, mc::EPI_BF16, nullptr, s, &a8));
  }
  if (phases & 2)
    for (int i = 0; i < n; ++i) {
      // the image range of a block with a live image prompt: the IP attention reads the raw q this head norm is about to rotate
      if (!e->dimg.empty() && r[i].w >= e->dimg.data() && r[i].w < e->dimg.data() + e->dimg.size())
        MC_TRY(ip_attend(e, (int)(r[i].w - e->dimg.data()), s));
      HIP_TRY(mc::launch_headnorm_rope(qkv + (size_t)r[i].row0 * 3 * d, 3 * d, d, r[i].w->qn, r[i].w->kn, 1e-6f, e->cs, r[i].row0,
                                       r[i].rows, e->H, s));
    }
  return MC_OK;
}

// ... and after it: output projection (+gated residual), LN + modulate, MLP (+gated residual)
// capture_to != null (the LAST block of a model without single blocks): the MagCache residual R = x_new - x0 of the ranges'
// rows fused into the MLP-out epilogue (joint row index; the text rows of R are scratch, as in the single blocks)
mc_status double_post(const mc_mmdit* e, const Range* r, int n, hipStream_t s, float* capture_to) {
  const int d = e->d;
  bf16_t* xn = e->buf<bf16_t>("xn");
  bf16_t* am = e->buf<bf16_t>("am");
  const float* mod_b = n == 2 ? r[1].mod : nullptr;
  mc::GemmParams o = {}, f2 = {};
  MxRows a_o = {}, a_f1 = {}, a_f2 = {};
  if (r[0].w->o.mx) {   // mode 3: the attention output rows, quantised
    const MxDst to = mx_at(e, r[0].row0, r[0].rows, 0, true);
    a_o = to.rows();
    MC_TRY(mx_quantise(e, am + (size_t)r[0].row0 * 5 * d, 5 * d, r[0].rows, d, to, s));
  }
  const int epi_o = resid_epi(e, o, r[0].row0, r[0].mod + 2 * d, nullptr);
  MC_TRY(range_linear(e, r, n, &Stream::o, am + (size_t)r[0].row0 * 5 * d, 5 * d, o, epi_o, mod_b ? mod_b + 2 * d : nullptr, s, &a_o));
  for (int i = 0; i < n; ++i)
    MC_TRY(ln_for_linear(e, r[i].w->fc1, r[i].row0, r[i].rows, r[i].mod + 4 * d, r[i].mod + 3 * d, &a_f1, s));
  for (int i = 0; i < n; ++i) {
    mc::GemmParams f1 = {};
    f1.Cb = am + (size_t)r[i].row0 * 5 * d + d; f1.ldc = 5 * d;
    int epi_f1 = mc::EPI_GELU_BF16;
    if (r[i].w->fc2.mx) {   // MLP-out's operand: "aq"[:, d:5d], written by MLP-in's epilogue or quantised from "am"[:, d:5d]
      const MxDst to = mx_at(e, r[i].row0, r[i].rows, d);
      a_f2 = to.rows();
      if (r[i].w->fc1.mx && fused_quant(e)) {
        f1.Cq = to.q; f1.ldcq = to.ld; f1.c_mx = to.mx; f1.mx_rows_c = to.rows_pad;
        epi_f1 = gelu_quant_epi(e);
      }
    }
    MC_TRY(linear(e, r[i].w->fc1, r[i].rows, xn + (size_t)r[i].row0 * d, d, f1, epi_f1, s, nullptr, 0, nullptr, &a_f1));
    if (r[i].w->fc2.mx && epi_f1 == mc::EPI_GELU_BF16) {
      const MxDst to = mx_at(e, r[i].row0, r[i].rows, d);
      MC_TRY(mx_quantise(e, am + (size_t)r[i].row0 * 5 * d + d, 5 * d, r[i].rows, 4 * d, to, s));
    }
  }
  const int epi_f2 = resid_epi(e, f2, r[0].row0, r[0].mod + 5 * d, capture_to);
  return range_linear(e, r, n, &Stream::fc2, am + (size_t)r[0].row0 * 5 * d + d, 5 * d, f2, epi_f2, mod_b ? mod_b + 5 * d : nullptr, s,
                      &a_f2);
}

// Image stream and text stream of a double block touch disjoint rows of every buffer: with "mmdit_two_streams" the text
// half runs on the engine's side stream between a fork and a join event (capturable: the side stream joins back).
template <class FI, class FT>
mc_status run_two(mc_mmdit* e, hipStream_t s, int mode, FI&& img_part, FT&& txt_part) {
  const bool by_shape = mode < 0 && (long)e->Lt * 16 >= (long)e->Li && e->P == 1;
  if (!(by_shape || mode == 1 || mode == 2) || !e->side) {   // > 2: diagnostic modes split block_pre only
    MC_TRY(img_part(s));
    return txt_part(s);
  }
  const int i = e->ev_i;
  e->ev_i = (e->ev_i + 1) & 7;
  if (mode == 2) {   // diagnostic: same streams and events, but the text half starts after the image half
    MC_TRY(img_part(s));
    HIP_TRY(hipEventRecord(e->ev_fork[i], s));
    HIP_TRY(hipStreamWaitEvent(e->side, e->ev_fork[i], 0));
  } else {
    HIP_TRY(hipEventRecord(e->ev_fork[i], s));
    HIP_TRY(hipStreamWaitEvent(e->side, e->ev_fork[i], 0));
    MC_TRY(img_part(s));
  }
  MC_TRY(txt_part(e->side));
  HIP_TRY(hipEventRecord(e->ev_join[i], e->side));
  HIP_TRY(hipStreamWaitEvent(s, e->ev_join[i], 0));
  return MC_OK;
}

}  // namespace

// ================================================================================================ forward, in phases
// begin (conditioning, embeds) -> for every block: block_pre, [caller: all-gather of the image K|V shards], block_post
// -> end (final layer).  mc_mmdit_forward runs them back to back on one GPU.
namespace {

mc_status begin_impl(mc_mmdit* e, const float* img_dev, double timestep, double guidance, const float* txt_dev,
                     int txt_valid, const float* vec_dev, mc_mode mode, int branch, mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!e) return fail(MC_EINVAL, "null engine");
  MC_TRY(mc::check_ready(e->work, e->weights, "mc_mmdit_set_workspace"));
  if (e->weights.dirty()) return fail(MC_ESTATE, "LoRA adapters, scales or a touched weight changed: call mc_mmdit_lora_apply first");
  const mc_mmdit_config& c = e->cfg;
  const bool hy = c.family == MC_FAMILY_HUNYUAN;
  const bool qw = c.family == MC_FAMILY_QWEN;
  if (!img_dev || !txt_dev || (!vec_dev && !qw)) return fail(MC_EINVAL, "null input");
  if ((hy || qw) && (txt_valid <= 0 || txt_valid > e->Lt))
    return fail(MC_EINVAL, "txt_valid %d out of (0, %d]", txt_valid, e->Lt);
  if (branch < 0 || branch > (qw ? 1 : 0))
    return fail(MC_EINVAL, "CFG branch %d: this family has %s", branch, qw ? "branches 0 and 1" : "branch 0 only");
  if (mode == MC_MODE_SKIP && !e->have_res[branch])
    return fail(MC_ESTATE, "skip requested but the residual cache is empty");
  if (mode == MC_MODE_CALIB && !c.calibration) return fail(MC_ESTATE, "engine was created without calibration");
  if (mode == MC_MODE_CALIB && e->P > 1) return fail(MC_ESTATE, "calibration runs on one GPU in this engine");
  e->mode = mode;
  e->branch = branch;
  e->txt_valid = (hy || qw) ? txt_valid : e->Lt;
  e->begun = true;
  e->dst = (mode == MC_MODE_CALIB && e->have_res[branch]) ? 1 - e->res_cur[branch] : e->res_cur[branch];
  const int d = e->d, Li = e->Li, Lt = e->Lt, S = e->S, Sp = e->Sp;
  float* x = e->buf<float>("x");
  bf16_t* x0 = e->buf<bf16_t>("x0") + (size_t)e->img0 * d;   // image rows of the joint-indexed copy
  bf16_t* qkv = e->buf<bf16_t>("qkv");
  float* vecs = e->buf<float>("vecs");
  float* emod = e->buf<float>("emod");
  float *sin_t = vecs, *sin_g = vecs + d, *hid = vecs + 2 * d, *vec = vecs + 3 * d;
  if (!e->pads_clean) {
    // rows [S, S_pad) are read by the attention kernel (masked keys, ignored queries) and never written by a GEMM
    HIP_TRY(hipMemsetAsync(qkv, 0, e->work.find("qkv")->bytes, s));
    HIP_TRY(hipMemsetAsync(x + (size_t)S * d, 0, (size_t)(Sp - S) * d * 4, s));
    if (e->P > 1) HIP_TRY(hipMemsetAsync(e->buf<bf16_t>("kv_gather"), 0, e->work.find("kv_gather")->bytes, s));
    e->pads_clean = true;
  }
  // ---- conditioning vector: time + guidance + pooled text   (flux :303-313, hunyuan :53-67)
  // (Qwen-Image, QwenTimestepProjEmbeddings: the timestep MLP alone, no guidance and no pooled text)
  HIP_TRY(mc::launch_sinusoid(nullptr, timestep, 256, sin_t, s));
  MC_TRY(run_mlp2(e->time_mlp, sin_t, hid, vec, 0, s));
  if (!qw) {
    HIP_TRY(mc::launch_sinusoid(nullptr, guidance, 256, sin_g, s));
    MC_TRY(run_mlp2(e->guid_mlp, sin_g, hid, vec, 1, s));
    MC_TRY(run_mlp2(e->vec_mlp, vec_dev, hid, vec, 1, s));
  }
  // modulation of every block = Linear(silu(vec)); a skipped step needs the final layer's only
  if (mode == MC_MODE_SKIP) {
    const size_t r0 = e->mod_final();
    HIP_TRY(mc::launch_gemv_bf16w(e->mod.w + r0 * d, vec, e->mod.b + r0, emod + r0, 2 * d, d, 1, 0, 0, s));
  } else {
    HIP_TRY(mc::launch_gemv_bf16w(e->mod.w, vec, e->mod.b, emod, (int)e->mod_rows, d, 1, 0, 0, s));
  }
  // ---- image embedding of THIS rank's tokens: x_img = x_embedder(tokens) / img_in(latent); ori copy for MagCache
  {
    bf16_t* tokens = e->buf<bf16_t>("tokens");
    if (hy) {
      if (e->Kp != e->Kin) HIP_TRY(hipMemsetAsync(tokens, 0, (size_t)align_up(Li, 256) * e->Kp * 2, s));
      HIP_TRY(mc::launch_patchify(img_dev, c.in_channels, c.latent_f, c.latent_h, c.latent_w, e->tok0, Li, Li, tokens,
                                  e->Kp, s));
    } else {
      HIP_TRY(mc::launch_cast_pad_bf16(img_dev + (size_t)e->tok0 * e->Kin, e->Kin, Li, Li, e->Kin, tokens, e->Kp, s));
    }
    mc::GemmParams p = {};
    p.X = x + (size_t)e->img0 * d; p.ldx = d; p.X0out = x0; p.ldx0out = d; p.m_valid = Li;
    MC_TRY(linear(e, e->img_in, Li, tokens, e->Kp, p, mc::EPI_EMBED, s));
  }
  if (mode != MC_MODE_SKIP) {
    // ---- text embedding -> text rows of x   (flux :314; hunyuan :72-78 incl. the token refiner); replicated per rank
    // Qwen-Image (upstream forward, run on every call as the reference does :186-188): txt_norm = weighted RMSNorm
    // (eps 1e-6) of the txt_valid rows to bf16, the padded rows zero -- and zero after txt_in (m_valid)
    bf16_t* tin = e->buf<bf16_t>("txt_in");
    if (qw) {
      HIP_TRY(mc::launch_rmsnorm_rows_bf16(txt_dev, c.txt_dim, e->w_txt_norm, 1e-6f, tin, c.txt_dim, txt_valid, Lt, c.txt_dim, s));
    } else {
      HIP_TRY(mc::launch_cast_pad_bf16(txt_dev, c.txt_dim, Lt, Lt, c.txt_dim, tin, c.txt_dim, s));
    }
    mc::GemmParams p = {};
    p.X = x + (size_t)e->txt0 * d; p.ldx = d; p.X0out = e->buf<bf16_t>("txt_e"); p.ldx0out = d;
    p.m_valid = qw ? txt_valid : Lt;
    MC_TRY(linear(e, e->txt_in, Lt, tin, c.txt_dim, p, mc::EPI_EMBED, s));
    if (hy) MC_TRY(run_refiner(e, txt_dev, txt_valid, vecs, s));
  }
  return MC_OK;
}

// ControlNet (flux :374-384, :416-423): the sample block `blk` adds to its image rows, or null (the lists were checked
// against mc_mmdit_controlnet_index when they were set; blocks_repeat is a rule of the double blocks only)
const void* controlnet_sample(const mc_mmdit* e, int blk) {
  const bool dbl = blk < e->cfg.n_double;
  const std::vector<const void*>& v = dbl ? e->cn_double : e->cn_single;
  if (v.empty()) return nullptr;
  return dbl ? v[mc_mmdit_controlnet_index(e->cfg.n_double, (int)v.size(), blk, e->cn_repeat)]
             : v[mc_mmdit_controlnet_index(e->cfg.n_single, (int)v.size(), blk - e->cfg.n_double, 0)];
}

// x_img += sample rows of this rank.  The LAST block's output GEMM then leaves the residual capture to this launch
// (with_capture): the reference takes hidden_states - ori AFTER the add (:426), and (x + s) - x0 is not (x - x0) + s in
// fp32, so the kernel writes R = x_new - x0 itself.
mc_status controlnet_add(const mc_mmdit* e, const void* sample, bool with_capture, hipStream_t s) {
  const int d = e->d;
  const size_t elem = e->cn_dtype == MC_BF16 ? 2 : 4;
  const void* rows = static_cast<const char*>(sample) + (size_t)e->tok0 * d * elem;
  HIP_TRY(mc::launch_add_rows(e->buf<float>("x") + (size_t)e->img0 * d, d, rows, e->cn_dtype == MC_BF16,
                              with_capture ? e->residual(e->dst, e->branch) : nullptr, d,
                              with_capture ? e->buf<bf16_t>("x0") + (size_t)e->img0 * d : nullptr, d, e->Li, d, s));
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_mmdit_controlnet_index(int n_blocks, int n_samples, int block, int blocks_repeat) {
  if (n_blocks <= 0 || n_samples <= 0 || n_samples > n_blocks || block < 0 || block >= n_blocks) return -1;
  const int k = blocks_repeat ? block % n_samples : block / ((n_blocks + n_samples - 1) / n_samples);
  return k < n_samples ? k : -1;   // the reference raises IndexError past the end of its list
}

mc_status mc_mmdit_set_controlnet(mc_mmdit* e, const void* const* double_samples_dev, int n_double_samples,
                                  const void* const* single_samples_dev, int n_single_samples, mc_dtype dtype,
                                  int blocks_repeat) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->cfg.family != MC_FAMILY_FLUX) return fail(MC_EINVAL, "ControlNet residuals are a FLUX input; this engine is another family");
  if (e->begun) return fail(MC_ESTATE, "mc_mmdit_set_controlnet between mc_mmdit_begin and mc_mmdit_end");
  if (dtype != MC_F32 && dtype != MC_BF16) return fail(MC_EINVAL, "ControlNet samples are fp32 or bf16");
  const void* const* lists[2] = {double_samples_dev, single_samples_dev};
  const int counts[2] = {n_double_samples, n_single_samples}, blocks[2] = {e->cfg.n_double, e->cfg.n_single};
  for (int k = 0; k < 2; ++k) {
    const int m = counts[k], n = blocks[k];
    const char* what = k ? "single" : "double";
    if (m < 0 || (m > 0 && !lists[k])) return fail(MC_EINVAL, "ControlNet: %d %s samples with a null list", m, what);
    if (m > n) return fail(MC_EINVAL, "ControlNet: %d samples for %d %s blocks", m, n, what);
    for (int i = 0; i < n && m > 0; ++i)
      if (mc_mmdit_controlnet_index(n, m, i, k == 0 && blocks_repeat) < 0)
        return fail(MC_EINVAL, "ControlNet: %d samples leave %s block %d of %d without one", m, what, i, n);
    for (int i = 0; i < m; ++i)
      if (!lists[k][i] || (reinterpret_cast<uintptr_t>(lists[k][i]) & 15))
        return fail(MC_EINVAL, "ControlNet: %s sample %d is null or not 16-byte aligned", what, i);
  }
  e->cn_double.assign(double_samples_dev, double_samples_dev + n_double_samples);
  e->cn_single.assign(single_samples_dev, single_samples_dev + n_single_samples);
  e->cn_dtype = dtype;
  e->cn_repeat = blocks_repeat != 0;
  return MC_OK;
}

// ---- IP-Adapters
static mc_status ip_entry(const mc_mmdit* e, const char* what) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->cfg.family != MC_FAMILY_FLUX) return fail(MC_EINVAL, "%s: IP-Adapters are a FLUX input; this engine is another family", what);
  if (e->begun) return fail(MC_ESTATE, "%s between mc_mmdit_begin and mc_mmdit_end", what);
  return MC_OK;
}
static mc_status ip_which(const mc_mmdit* e, int adapter) {
  if (adapter < 0 || adapter >= (int)e->ip.size()) return fail(MC_EINVAL, "IP-Adapter %d of %zu", adapter, e->ip.size());
  return MC_OK;
}

mc_status mc_mmdit_ip_adapter_add(mc_mmdit* e, int embed_dim, int cross_dim, int tokens_per_image, int* index) {
  MC_TRY(ip_entry(e, "mc_mmdit_ip_adapter_add"));
  if (e->cfg.n_double == 0) return fail(MC_EINVAL, "IP-Adapter: the engine has no double blocks");
  if ((int)e->ip.size() >= mc::kIpMaxAdapters) return fail(MC_EINVAL, "IP-Adapter: at most %d adapters", mc::kIpMaxAdapters);
  static const int ln_ok[] = {1, 2, 4, 5, 6, 8, 12, 16, 20};   // launch_ln_modulate's widths, in units of 256
  bool cross_ok = cross_dim > 0 && (cross_dim % 256) == 0;
  if (cross_ok) { cross_ok = false; for (int v : ln_ok) cross_ok |= v == cross_dim / 256; }
  if (!cross_ok) return fail(MC_EINVAL, "IP-Adapter: cross_dim %d is no LayerNorm width of this library (256 x 1, 2, 4, 5, 6, 8, 12, 16, 20)", cross_dim);
  if (embed_dim <= 0 || (embed_dim % 8) != 0 || embed_dim > 16384) return fail(MC_EINVAL, "IP-Adapter: embed_dim %d (a multiple of 8, at most 16384)", embed_dim);
  if (tokens_per_image < 1 || tokens_per_image > mc::kIpMaxKeys) return fail(MC_EINVAL, "IP-Adapter: %d tokens per image (1..%d)", tokens_per_image, mc::kIpMaxKeys);
  const int j = (int)e->ip.size();
  const size_t d = e->d;
  mc::WeightStore& W = e->weights;
  if (cross_dim > e->ip_h_cross) {   // the scratch of set_image: kIpMaxKeys rows of the widest adapter
    float* h32 = nullptr; bf16_t* hb = nullptr;
    MC_TRY(W.alloc(&h32, (size_t)mc::kIpMaxKeys * cross_dim));
    if (mc_status st = W.alloc(&hb, (size_t)mc::kIpMaxKeys * cross_dim)) { W.release(h32); return st; }
    HIP_TRY(hipMemset(hb, 0, (size_t)mc::kIpMaxKeys * cross_dim * 2));
    if (e->ip_h32) { W.release(e->ip_h32); W.release(e->ip_hb); }
    e->ip_h32 = h32; e->ip_hb = hb; e->ip_h_cross = cross_dim;
  }
  MC_TRY(ip_grow_out(e, e->Li));
  auto a = std::make_unique<IpAdapter>();
  a->embed_dim = embed_dim; a->cross_dim = cross_dim; a->tokens = tokens_per_image;
  a->scale.assign(e->cfg.n_double, 1.f);
  a->kv.resize(e->cfg.n_double);
  const std::string js = std::to_string(j), pp = "encoder_hid_proj.image_projection_layers." + js + ".";
  MC_TRY(W.add_linear(a->proj, pp, {{"image_embeds", (size_t)tokens_per_image * cross_dim}}, embed_dim));
  MC_TRY(W.add_f32(a->ln_w, pp + "norm.weight", cross_dim));
  MC_TRY(W.add_f32(a->ln_b, pp + "norm.bias", cross_dim));
  a->names = {pp + "image_embeds.weight", pp + "image_embeds.bias", pp + "norm.weight", pp + "norm.bias"};
  for (int i = 0; i < e->cfg.n_double; ++i) {
    const std::string p = "transformer_blocks." + std::to_string(i) + ".attn.processor.";
    MC_TRY(W.add_linear(a->kv[i], p, {{"to_k_ip." + js, d}, {"to_v_ip." + js, d}}, cross_dim));
    for (const char* part : {"to_k_ip.", "to_v_ip."})
      for (const char* leaf : {".weight", ".bias"}) a->names.push_back(p + part + js + leaf);
  }
  e->ip.push_back(std::move(a));
  if (index) *index = j;
  return MC_OK;
}

mc_status mc_mmdit_ip_adapter_set_image(mc_mmdit* e, int adapter, int slot, const float* embeds_dev, int n_images, mc_stream stream) {
  MC_TRY(ip_entry(e, "mc_mmdit_ip_adapter_set_image"));
  MC_TRY(ip_which(e, adapter));
  if (slot < 0 || slot > 1) return fail(MC_EINVAL, "IP-Adapter image slot %d (0 or 1)", slot);
  IpAdapter& a = *e->ip[adapter];
  if (n_images == 0) { a.keys[slot] = 0; return MC_OK; }
  const int keys = n_images * a.tokens;
  if (n_images < 0 || n_images > mc::kIpMaxKeys || keys > mc::kIpMaxKeys)
    return fail(MC_EINVAL, "IP-Adapter %d: %d images of %d tokens are more than %d keys", adapter, n_images, a.tokens, mc::kIpMaxKeys);
  if (!embeds_dev || (reinterpret_cast<uintptr_t>(embeds_dev) & 15)) return fail(MC_EINVAL, "IP-Adapter: the image embeds are null or not 16-byte aligned");
  for (const std::string& n : a.names)
    if (!e->weights.slots.at(n).loaded) return fail(MC_ESTATE, "IP-Adapter %d: weight '%s' is not set", adapter, n.c_str());
  hipStream_t s = (hipStream_t)stream;
  const size_t d = e->d;
  if (keys > a.rows[slot]) {   // the slot's cache grows: an earlier forward may still read the old one
    HIP_TRY(hipDeviceSynchronize());
    const int rows = (int)align_up(keys, 32);
    bf16_t* grown = nullptr;
    MC_TRY(e->weights.alloc(&grown, (size_t)e->cfg.n_double * rows * 2 * d));
    if (a.cache[slot]) e->weights.release(a.cache[slot]);
    a.cache[slot] = grown;
    a.rows[slot] = rows;
  }
  a.keys[slot] = 0;   // until everything below is launched
  // ImageProjection: Linear per image (its [tokens * cross_dim] output is tokens rows of the hidden states), affine LayerNorm
  const int row_w = a.tokens * a.cross_dim;
  for (int i = 0; i < n_images; ++i)
    HIP_TRY(mc::launch_gemv_bf16w(a.proj.w, embeds_dev + (size_t)i * a.embed_dim, a.proj.b, e->ip_h32 + (size_t)i * row_w, row_w, a.embed_dim,
                                  0, 0, 0, s));
  HIP_TRY(mc::launch_ln_modulate(e->ip_h32, a.cross_dim, nullptr, 0, a.ln_w, a.ln_b, 1, 1e-5f, e->ip_hb, a.cross_dim, nullptr, 0, keys,
                                 a.cross_dim, s));
  for (int i = 0; i < e->cfg.n_double; ++i) {
    mc::GemmParams p = {};
    p.Cb = a.cache[slot] + (size_t)i * a.rows[slot] * 2 * d; p.ldc = 2 * d;
    // not through linear(): no split-K scratch of the workspace, so that a slot's bits depend on no geometry and no forward
    // on another stream shares scratch with this call
    HIP_TRY(mc::launch_linear_bf16(a.kv[i], mc::whole(a.kv[i]), e->ip_hb, a.cross_dim, keys, p, mc::EPI_BF16, s));
  }
  a.keys[slot] = keys;
  return MC_OK;
}

mc_status mc_mmdit_ip_adapter_scale(mc_mmdit* e, int adapter, const float* scales, int n) {
  MC_TRY(ip_entry(e, "mc_mmdit_ip_adapter_scale"));
  MC_TRY(ip_which(e, adapter));
  if (!scales || (n != 1 && n != e->cfg.n_double)) return fail(MC_EINVAL, "IP-Adapter scales: 1 or %d values, %d given", e->cfg.n_double, n);
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(scales[i])) return fail(MC_EINVAL, "IP-Adapter scale %d is not finite", i);
  IpAdapter& a = *e->ip[adapter];
  for (int i = 0; i < e->cfg.n_double; ++i) a.scale[i] = scales[n == 1 ? 0 : i];
  return MC_OK;
}

mc_status mc_mmdit_ip_adapter_select(mc_mmdit* e, int slot) {
  MC_TRY(ip_entry(e, "mc_mmdit_ip_adapter_select"));
  if (slot < -1 || slot > 1) return fail(MC_EINVAL, "IP-Adapter image slot %d (-1: none, 0, 1)", slot);
  e->ip_slot = slot;
  return MC_OK;
}

mc_status mc_mmdit_ip_adapter_clear(mc_mmdit* e) {
  MC_TRY(ip_entry(e, "mc_mmdit_ip_adapter_clear"));
  if (e->ip.empty()) { e->ip_slot = -1; return MC_OK; }
  HIP_TRY(hipDeviceSynchronize());   // an earlier forward may still read what goes
  for (auto& a : e->ip) {
    for (const std::string& n : a->names) e->weights.slots.erase(n);
    e->weights.release(a->proj.w); e->weights.release(a->proj.b);
    e->weights.release(a->ln_w); e->weights.release(a->ln_b);
    for (Linear& l : a->kv) { e->weights.release(l.w); e->weights.release(l.b); }
    for (bf16_t* c : a->cache) if (c) e->weights.release(c);
  }
  e->ip.clear();
  e->ip_slot = -1;
  return MC_OK;
}

mc_status mc_mmdit_begin(mc_mmdit* e, const float* img_dev, double timestep, double guidance, const float* txt_dev,
                         int txt_valid, const float* vec_dev, mc_mode mode, mc_stream stream) {
  return begin_impl(e, img_dev, timestep, guidance, txt_dev, txt_valid, vec_dev, mode, 0, stream);
}

// block index: 0 .. n_double-1 double-stream blocks, then the single-stream blocks
mc_status mc_mmdit_block_pre(mc_mmdit* e, int blk, mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!e || !e->begun) return fail(MC_ESTATE, "mc_mmdit_begin must run first");
  const mc_mmdit_config& c = e->cfg;
  if (blk < 0 || blk >= c.n_double + c.n_single) return fail(MC_EINVAL, "block %d out of range", blk);
  const int d = e->d, Li = e->Li, S = e->S;
  const float* emod = e->buf<float>("emod");
  bf16_t* qkv = e->buf<bf16_t>("qkv");
  if (blk < c.n_double) {
    const TwoStreams t = two_streams(e, blk, emod);
    auto img = [&](hipStream_t q, int ph) { return double_pre(e, &t.r[t.img], 1, q, ph); };
    auto txt = [&](hipStream_t q, int ph) { return double_pre(e, &t.r[t.txt], 1, q, ph); };
    const int mode = g_mmdit_two_streams;
    if (e->fp8) {   // one range at a time, in row order, on the launch stream whatever "mmdit_two_streams" says
      MC_TRY(double_pre(e, &t.r[0], 1, s));
      MC_TRY(double_pre(e, &t.r[1], 1, s));
    } else if (double_block_merged(e)) {
      MC_TRY(double_pre(e, t.r, 2, s));
    } else if (mode <= 2) {
      MC_TRY(run_two(e, s, mode, [&](hipStream_t q) { return img(q, 3); }, [&](hipStream_t q) { return txt(q, 3); }));
    } else {   // diagnostic splits: which pair of kernels must overlap for the results to change
      mc_status st = MC_OK;
      if (mode == 3) {          // text LN + GEMM beside the image half; text head norm afterwards, serial
        st = run_two(e, s, 1, [&](hipStream_t q) { return img(q, 3); }, [&](hipStream_t q) { return txt(q, 1); });
        if (st == MC_OK) st = txt(s, 2);
      } else if (mode == 4) {   // text LN + GEMM first, serial; text head norm beside the whole image half
        st = txt(s, 1);
        if (st == MC_OK) st = run_two(e, s, 1, [&](hipStream_t q) { return img(q, 3); }, [&](hipStream_t q) { return txt(q, 2); });
      } else if (mode == 5) {   // image LN + GEMM beside the whole text half; image head norm afterwards, serial
        st = run_two(e, s, 1, [&](hipStream_t q) { return img(q, 1); }, [&](hipStream_t q) { return txt(q, 3); });
        if (st == MC_OK) st = img(s, 2);
      } else {                  // 6: LN + GEMM of both halves serial; the two head norm kernels beside each other
        st = img(s, 1);
        if (st == MC_OK) st = txt(s, 1);
        if (st == MC_OK) st = run_two(e, s, 1, [&](hipStream_t q) { return img(q, 2); }, [&](hipStream_t q) { return txt(q, 2); });
      }
      MC_TRY(st);
    }
  } else {
    const int i = blk - c.n_double;
    const Single& g = e->singles[i];
    const float* m = emod + e->mod_single(i);
    bf16_t* xn = e->buf<bf16_t>("xn");
    bf16_t* am = e->buf<bf16_t>("am");
    MxRows a8 = {};
    MC_TRY(ln_for_linear(e, g.in, 0, S, m + d, m, &a8, s));
    mc::GemmParams p = {};
    p.Cb = qkv; p.ldc = 3 * d;
    if (g.in.mx) {
      // MX has no two-destination epilogue: two launches over row ranges of the fused weight, q|k|v into "qkv" and the GELU'd
      // MLP-in columns into "am"[:, d:] -- or, mode 3 with fused quantisers, straight into the output projection's operand
      MC_TRY(linear(e, g.in, S, nullptr, 0, p, mc::EPI_BF16, s, nullptr, 0, nullptr, &a8, {0, 3 * d}));
      mc::GemmParams f = {};
      f.Cb = am + d; f.ldc = 5 * d;
      int epi = mc::EPI_GELU_BF16;
      if (g.out.mx && fused_quant(e)) {
        const MxDst to = mx_at(e, 0, S, d);
        f.Cq = to.q; f.ldcq = to.ld; f.c_mx = to.mx; f.mx_rows_c = to.rows_pad;
        epi = gelu_quant_epi(e);
      }
      MC_TRY(linear(e, g.in, S, nullptr, 0, f, epi, s, nullptr, 0, nullptr, &a8, {3 * d, 4 * d}));
    } else {
      // linear1 of the single block = [q | k | v ; MLP-in] over the same rows: ONE launch with two destinations (the q|k|v
      // columns to "qkv", the GELU'd MLP columns to "am"[:, d:]) -- 504 tiles at FLUX 512^2 are two trips of the 256 CUs, the
      // two launches were 216 + 288 = one + two
      p.n_split = 3 * d; p.Cb2 = am + d; p.ldc2 = 5 * d;
      MC_TRY(linear(e, g.in, S, xn, d, p, mc::EPI_BF16_GELU_SPLIT, s));
    }
    HIP_TRY(mc::launch_headnorm_rope(qkv, 3 * d, d, g.qn, g.kn, 1e-6f, e->cs, 0, S, e->H, s));
  }
  if (e->P > 1) {
    // this rank's image K|V rows -> its slot of the gather buffer ([P][Lr_pad][2d]; the caller all-gathers it)
    bf16_t* slot = e->buf<bf16_t>("kv_gather") + (size_t)e->rank * e->Lrp * 2 * d;
    HIP_TRY(hipMemcpy2DAsync(slot, (size_t)2 * d * 2, qkv + (size_t)e->img0 * 3 * d + d, (size_t)3 * d * 2, (size_t)2 * d * 2,
                             Li, hipMemcpyDeviceToDevice, s));
  }
  return MC_OK;
}

// optional, sp_size > 1: attention of the local queries over THIS rank's image shard and the (replicated) text keys --
// everything that needs nothing from the other ranks -- to be launched while the all-gather is in flight; the
// following mc_mmdit_block_post then attends the remote image shards only and merges.
mc_status mc_mmdit_block_attn_local(mc_mmdit* e, int blk, mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!e || !e->begun) return fail(MC_ESTATE, "mc_mmdit_begin must run first");
  if (e->P < 2) return fail(MC_ESTATE, "mc_mmdit_block_attn_local needs sp_size > 1");
  float* lse = e->buf<float>("attn_lse");
  MC_TRY(attend(e, e->Sp, image_keys(e), nullptr, lse, s));   // this rank's shard: rows of the local qkv
  MC_TRY(attend(e, e->Sp, text_keys(e), lse, lse, s));
  e->local_attn_blk = blk;
  return MC_OK;
}

mc_status mc_mmdit_block_post(mc_mmdit* e, int blk, mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!e || !e->begun) return fail(MC_ESTATE, "mc_mmdit_begin must run first");
  const mc_mmdit_config& c = e->cfg;
  const int nb = c.n_double + c.n_single;
  if (blk < 0 || blk >= nb) return fail(MC_EINVAL, "block %d out of range", blk);
  const int d = e->d, Li = e->Li, Lt = e->Lt, S = e->S, Sp = e->Sp;
  const float* emod = e->buf<float>("emod");
  // ---- joint attention of the local queries over [all image tokens ; valid text tokens]
  if (e->P == 1 && c.family == MC_FAMILY_QWEN && e->txt_valid < Lt) {
    // Qwen-Image with a prompt shorter than txt_len: the image keys (log-sum-exp kept), then the txt_valid text keys merged
    // with it -- the padded text rows [txt_valid, txt_len) are never keys
    float* lse = e->buf<float>("attn_lse");
    MC_TRY(attend(e, Sp, image_keys(e), nullptr, lse, s));
    MC_TRY(attend(e, Sp, text_keys(e), lse, nullptr, s));
  } else if (e->P == 1) {   // all S rows of qkv are keys (HunyuanVideo: its valid text rows are the last of them)
    MC_TRY(attend(e, Sp, local_keys(e, 0, Sp, c.family == MC_FAMILY_HUNYUAN ? Li + e->txt_valid : S), nullptr, nullptr, s));
  } else if (e->local_attn_blk == blk) {   // mc_mmdit_block_attn_local did the local shard and the text keys: the remote shards, merged
    e->local_attn_blk = -1;
    MC_TRY(attend(e, Sp, gathered_keys(e, e->rank + 1), e->buf<float>("attn_lse"), nullptr, s));
  } else {
    // (1) the image keys of every rank (gathered shards of Li rows), (2) the text keys (replicated, local rows of qkv),
    // merged with the log-sum-exp of (1) in the kernel epilogue
    float* lse = e->buf<float>("attn_lse");
    MC_TRY(attend(e, Sp, gathered_keys(e, 0), nullptr, lse, s));
    MC_TRY(attend(e, Sp, text_keys(e), lse, nullptr, s));
  }
  const bool last = (blk == nb - 1);
  const void* cn = (e->cn_double.empty() && e->cn_single.empty()) ? nullptr : controlnet_sample(e, blk);
  const bool ip = ip_live(e, blk, nullptr) > 0;
  // the add that runs last on the last block captures after it: a ControlNet sample's, else the IP-Adapter's, else MLP-out
  const bool capture = last && !cn && !ip;
  float* capture_to = capture ? e->residual_joint(e->dst, e->branch) : nullptr;
  if (blk < c.n_double) {
    const TwoStreams t = two_streams(e, blk, emod);
    if (e->fp8) {
      MC_TRY(double_post(e, &t.r[0], 1, s, capture_to));
      MC_TRY(double_post(e, &t.r[1], 1, s, capture_to));
    } else if (double_block_merged(e)) {
      MC_TRY(double_post(e, t.r, 2, s, capture_to));
    } else {
      MC_TRY(run_two(
          e, s, g_mmdit_two_streams > 2 ? 0 : g_mmdit_two_streams,
          [&](hipStream_t q) { return double_post(e, &t.r[t.img], 1, q, capture_to); },
          [&](hipStream_t q) { return double_post(e, &t.r[t.txt], 1, q, nullptr); }));
    }
  } else {
    const int i = blk - c.n_double;
    mc::GemmParams o = {};   // MagCache residual capture (flux :428, hunyuan :140); the text rows of R are scratch
    const int epi = resid_epi(e, o, 0, emod + e->mod_single(i) + 2 * d, capture_to);
    const Single& g = e->singles[i];
    bf16_t* am = e->buf<bf16_t>("am");
    MxRows a8 = {};
    if (g.out.mx) {
      // mode 3: the K = 5d operand [attention | GELU(MLP-in)] in "aq"; with fused quantisers linear1's epilogue wrote the
      // GELU columns and their scales already, so only the attention columns are quantised here
      const MxDst to = mx_at(e, 0, S, 0);
      a8 = to.rows();
      MC_TRY(mx_quantise(e, am, 5 * d, S, (g.in.mx && fused_quant(e)) ? d : 5 * d, to, s));
    }
    MC_TRY(linear(e, g.out, S, am, 5 * d, o, epi, s, nullptr, 0, nullptr, &a8));
  }
  if (ip) {   // hidden_states + ip_attn_output (FluxTransformerBlock.forward): behind the MLP, in front of the ControlNet sample
    const bool cap = last && !cn;
    HIP_TRY(mc::launch_add_rows(e->buf<float>("x") + (size_t)e->img0 * d, d, e->ip_out, 1, cap ? e->residual(e->dst, e->branch) : nullptr,
                                d, cap ? e->buf<bf16_t>("x0") + (size_t)e->img0 * d : nullptr, d, Li, d, s));
  }
  if (cn) MC_TRY(controlnet_add(e, cn, last, s));
  if (last) {
    const int b = e->branch;   // calibration compares with the previous residual of the SAME branch
    if (e->mode == MC_MODE_CALIB && e->have_res[b]) {
      HIP_TRY(mc::launch_calib_stats(e->residual(e->dst, b), d, e->residual(e->res_cur[b], b), d, Li, d,
                                     e->buf<double>("calib_partial"), 2048, e->buf<double>("calib_sums"),
                                     e->buf<float>("calib_stats"), s));
      e->have_stats = true;
    }
    e->res_cur[b] = e->dst;
    e->have_res[b] = true;
  }
  return MC_OK;
}

// final layer on this rank's image tokens: AdaLN (no affine) + Linear   (flux :431-432, hunyuan :144).
// One GPU: out_dev = FLUX [img_tokens, out_channels] / HunyuanVideo [C, F, H, W].  sp_size > 1: FLUX writes its
// [img_tokens / P, out_channels] rows to out_dev; HunyuanVideo leaves its rows in "head_tokens" ([.., 64] fp32) for the
// caller to gather and hand to mc_mmdit_unpatchify (out_dev may be NULL).
mc_status mc_mmdit_end(mc_mmdit* e, float* out_dev, mc_stream stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!e || !e->begun) return fail(MC_ESTATE, "mc_mmdit_begin must run first");
  const mc_mmdit_config& c = e->cfg;
  const bool hy = c.family == MC_FAMILY_HUNYUAN;
  if (!out_dev && !(hy && e->P > 1)) return fail(MC_EINVAL, "null output");
  const int d = e->d, Li = e->Li;
  const float* mf = e->buf<float>("emod") + e->mod_final();
  const float* scale = hy ? mf + d : mf;   // hunyuan: (shift, scale); flux AdaLayerNormContinuous: (scale, shift)
  const float* shift = hy ? mf : mf + d;
  float* hn = reinterpret_cast<float*>(e->buf<bf16_t>("am"));
  bf16_t* x0 = e->buf<bf16_t>("x0") + (size_t)e->img0 * d;
  if (e->mode == MC_MODE_SKIP) {
    // hidden_states = ori + cur_residual (flux :348, hunyuan :102) folded into the LayerNorm load
    HIP_TRY(mc::launch_ln_modulate(e->residual(e->res_cur[e->branch], e->branch), d, x0, d, scale, shift, 0, 1e-6f, nullptr,
                                   0, hn, d, Li, d, s));
  } else {
    HIP_TRY(mc::launch_ln_modulate(e->buf<float>("x") + (size_t)e->img0 * d, d, nullptr, 0, scale, shift, 0, 1e-6f,
                                   nullptr, 0, hn, d, Li, d, s));
  }
  if (hy) {
    float* ht = e->buf<float>("head_tokens");
    HIP_TRY(mc::launch_head_linear(hn, d, e->w_head, e->b_head, ht, 64, Li, e->out_feat, d, s));
    if (e->P == 1)
      HIP_TRY(mc::launch_unpatchify(ht, 64, c.out_channels, c.latent_f, c.latent_h, c.latent_w, 0, Li, out_dev, s));
  } else {
    HIP_TRY(mc::launch_head_linear(hn, d, e->w_head, e->b_head, out_dev, e->out_feat, Li, e->out_feat, d, s));
  }
  e->begun = false;
  return MC_OK;
}

// HunyuanVideo, sp_size > 1: tokens_dev = the gathered head tokens [img_tokens, 64] fp32 -> out_dev [C, F, H, W]
mc_status mc_mmdit_unpatchify(mc_mmdit* e, const float* tokens_dev, float* out_dev, mc_stream stream_) {
  if (!e || !tokens_dev || !out_dev) return fail(MC_EINVAL, "null argument");
  const mc_mmdit_config& c = e->cfg;
  if (c.family != MC_FAMILY_HUNYUAN) return fail(MC_EINVAL, "FLUX returns tokens; there is nothing to unpatchify");
  HIP_TRY(mc::launch_unpatchify(tokens_dev, 64, c.out_channels, c.latent_f, c.latent_h, c.latent_w, 0, c.img_tokens,
                                out_dev, (hipStream_t)stream_));
  return MC_OK;
}

mc_status mc_mmdit_forward(mc_mmdit* e, const float* img_dev, double timestep, double guidance, const float* txt_dev,
                           int txt_valid, const float* vec_dev, mc_mode mode, float* out_dev, mc_stream stream) {
  return mc_mmdit_forward2(e, img_dev, timestep, guidance, txt_dev, txt_valid, vec_dev, mode, 0, out_dev, stream);
}

mc_status mc_mmdit_forward2(mc_mmdit* e, const float* img_dev, double timestep, double guidance, const float* txt_dev,
                            int txt_valid, const float* vec_dev, mc_mode mode, int branch, float* out_dev,
                            mc_stream stream) {
  if (!e) return fail(MC_EINVAL, "null engine");
  if (e->P != 1) return fail(MC_ESTATE, "mc_mmdit_forward is single-GPU; drive a sharded engine through the phase calls");
  if (!out_dev) return fail(MC_EINVAL, "null output");
  MC_TRY(begin_impl(e, img_dev, timestep, guidance, txt_dev, txt_valid, vec_dev, mode, branch, stream));
  if (mode != MC_MODE_SKIP) {
    for (int b = 0; b < e->cfg.n_double + e->cfg.n_single; ++b) {
      MC_TRY(mc_mmdit_block_pre(e, b, stream));
      MC_TRY(mc_mmdit_block_post(e, b, stream));
    }
  }
  return mc_mmdit_end(e, out_dev, stream);
}

}  // extern "C"
