// What the host-side engines (engine.cpp, mmdit_engine.cpp) share, internal like ops.h: the error text mc_last_error()
// reports, the named weight store behind *_set_weight, the workspace plan behind *_set_workspace, the Linear descriptor and
// the key set of an attention launch, each with its launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/magcache_hip.h"
#include "ops.h"

namespace mc {

// ---------------------------------------------------------------- error text (thread local, one per library)
mc_status fail(mc_status s, const char* fmt, ...);
const char* last_error();

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) return ::mc::fail(MC_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define MC_TRY(expr)                 \
  do {                               \
    mc_status _s = (expr);           \
    if (_s != MC_OK) return _s;      \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// mc_set_option values (ops_capi.cpp sets them), each defined in the file that reads it
extern int g_fp8_fused_quant;    // engine.cpp
extern int g_sp_attn_partials;   // engine.cpp
extern int g_mx_fp4;             // engine.cpp: read once, through latch_mx_format, by mc_create and by mc_mmdit_create / _create_sized
extern int g_mx_fp6;             // engine.cpp: the same for MXFP6; both 1 at create time is MC_EINVAL
extern int g_mmdit_two_streams;  // mmdit_engine.cpp

// ---------------------------------------------------------------- weights
// y = x W^T + b with W [n_out, k_in] bf16 and, optionally, an e4m3 copy of W made when the weight is set: with one scale
// per output channel (q_scale) or with MX block scales (mx: E8M0, block-major [k_in / 32][n_out]).  q == null: bf16 only.
// fmt (meaningful where mx != null): the element format of the MX copy -- packed rows of mx_row_bytes(fmt, k_in) bytes in q
// (ops.h: MxFormat), the same scale image for every format.
struct Linear {
  bf16_t* w = nullptr;
  float* b = nullptr;
  int n_out = 0, k_in = 0;
  uint8_t* q = nullptr;
  float* q_scale = nullptr;
  uint8_t* mx = nullptr;
  MxFormat fmt = MX_E4M3;
  bf16_t* w_base = nullptr;  // the pristine weight while a LoRA adapter touches this Linear (w is then the merged one)
  long q_row_bytes() const { return mx ? mx_row_bytes(fmt, k_in) : k_in; }   // of one row of q
};
// one scale per output channel | one E8M0 byte per (channel, 32 inputs), the elements in the MxFormat given beside it
enum Quant { QUANT_NONE, QUANT_ROW, QUANT_MX };
struct Part { std::string name; size_t rows; };   // an upstream Linear whose rows are stacked into a fused one (q | k | v -> qkv)
struct RowRange { int first, count; };            // output channels of a Linear: all of them, or k|v / q of the fused q|k|v
inline RowRange whole(const Linear& l) { return {0, l.n_out}; }

struct Slot {  // one named parameter
  void* dst = nullptr;
  mc_dtype dst_dtype = MC_F32;
  size_t numel = 0;
  size_t off = 0;  // element offset inside a fused destination (q/k/v -> wqkv)
  int perm_c = 0;  // > 0: rows are (c, pq) channel-major upstream and are stored (pq, c) -- HunyuanVideo final linear
  struct Pad { size_t rows = 0, k_in = 0, k_pitch = 0; } pad;  // rows > 0: given [rows, k_in], stored with row pitch k_pitch
  bool loaded = false;
  // quantised copy: after the bf16 store the same rows are quantised into q8 -- per output channel (q8_scale), or, mx != null,
  // relative to E8M0 block scales of the fused destination, block-major with mx_rows rows per k block
  uint8_t* q8 = nullptr;
  float* q8_scale = nullptr;
  size_t q8_k = 0;  // row length (in_features)
  uint8_t* mx = nullptr;
  size_t mx_rows = 0;
  MxFormat fmt = MX_E4M3;   // mx != null: the copy's element format, packed rows of mx_row_bytes(fmt, q8_k) bytes
  Linear* lin = nullptr;  // the Linear whose rows this weight is (add_parts); null for every other parameter
  // adapters on an fp32 parameter (WeightStore::allow_f32_targets)
  size_t f32_k = 0;           // > 0: an fp32 matrix [numel / f32_k, f32_k], which takes low-rank pairs; 0: deltas only
  float* f32_base = nullptr;  // its numel pristine elements while an adapter touches it (dst + off is then the merged value)
  bool fixed = false;         // takes no adapter whatever its layout (the Wan patch embedders)
};

// One adapter's term of one kind on one weight slot: device copies owned by the store, as the merge launches read them
// (ops.h: LoraTerm, KronTerm, HadaTerm, launch_param_delta).  (adapter, target, kind) names a term.
struct AdapterTerm {
  enum Kind { PAIR, DELTA, KRON, HADA, MAGNITUDE };
  std::string adapter, target;
  Kind kind = PAIR;
  float factor = 1.f;   // alpha / rank of the target (PAIR), the term's own factor (KRON, HADA); 1 for a DELTA and a MAGNITUDE
  // PAIR: up [rows x rank_pad], down_t [k_in x rank_pad], packed bf16 with the rank zero-padded to the kernel's step
  // DELTA: numel fp32 | KRON: w1, w2 fp32 | HADA: u1, d1, u2, d2 fp32 | MAGNITUDE: g [rows] fp32
  void* p[4] = {nullptr, nullptr, nullptr, nullptr};
  int rank_pad = 0, rank = 0, r1 = 0, c1 = 0, r2 = 0, c2 = 0;
  const float* f32(int i) const { return (const float*)p[i]; }
  // what the limit of kLoraMaxTerms counts together: the deltas of an fp32 parameter | the pairs, Kronecker and Hadamard
  // terms of a matrix; a magnitude never counts
  bool counts_with(Kind k) const { return kind != MAGNITUDE && k != MAGNITUDE && (kind == DELTA) == (k == DELTA); }
};
struct TermArrays;   // host.cpp: the launch arrays of one target

struct WeightStore {
  std::map<std::string, Slot> slots;
  std::vector<void*> owned;
  // the owning engine's opt-in (the Wan engine sets it at mc_create): fp32 matrices take pairs, fp32 parameters take deltas.
  // false: lora_set refuses every fp32 weight and lora_set_delta everything
  bool allow_f32_targets = false;

  template <class T>
  mc_status alloc(T** p, size_t n) { return alloc_bytes(reinterpret_cast<void**>(p), n * sizeof(T)); }
  Slot& add(const std::string& name, void* dst, mc_dtype dt, size_t numel, size_t off = 0);
  // an fp32 parameter that is no Linear's (norm weights, modulation, the fp32 matrices of a GEMV): allocates and registers it
  // (k_in > 0: a matrix [numel / k_in, k_in], Slot::f32_k)
  mc_status add_f32(float*& p, const std::string& name, size_t numel, size_t k_in = 0);
  // One Linear [sum of the parts' rows, k_in]: allocates the bf16 weight + fp32 bias (and, quant != QUANT_NONE, the quantised
  // copy with its scales; fmt: its element format where quant == QUANT_MX) and registers the parts.  alloc_linear / add_parts are its two halves, for a Linear whose parts are
  // added one by one (the fused modulation matrix) or whose slot the caller adjusts (Slot::pad, Slot::perm_c).
  mc_status add_linear(Linear& l, const std::string& prefix, const std::vector<Part>& parts, size_t k_in, Quant quant = QUANT_NONE,
                       MxFormat fmt = MX_E4M3);
  mc_status alloc_linear(Linear& l, size_t n_out, size_t k_in, Quant quant = QUANT_NONE, MxFormat fmt = MX_E4M3);
  // "<prefix><part>.weight" [rows, k_in] (bf16) and "<prefix><part>.bias" [rows] (fp32) of every part, stacked from row row0 of
  // `l`; every slot carries the quantised copy, so that setting a part requantises its rows.  Returns the last weight's slot.
  Slot& add_parts(Linear& l, const std::string& prefix, const std::vector<Part>& parts, size_t row0 = 0);
  // copy / cast / permute / pad one parameter into place (and requantise its rows) on the caller's stream
  mc_status set(const char* name, const void* src_dev, mc_dtype dtype, const int64_t* shape, int ndim, hipStream_t stream);
  // ---- LoRA adapters, merged into the live weight: w = bf16(w_base + sum_j scale_j factor_j up_j down_j) per touched part, in the
  // order the pairs were set.  Host bookkeeping + launches on the caller's stream; they may allocate and free (never inside a
  // forward, never under stream capture).  The forward reads the same pointers as ever.
  // Every lora_* call below is the whole body of its C entry point on either engine (mc_lora_* / mc_mmdit_lora_*): a null
  // argument is MC_EINVAL, shapes are the 2-D shapes the C calls take.
  // `weight_name`: a bf16 part of a Linear with no pad and no perm_c; down [rank, k_in], up [rows of the part, rank], fp32 or bf16.
  // The first pair on a Linear makes its base copy; setting (adapter, weight_name) again replaces the pair.  A new adapter
  // starts at scale 1.
  mc_status lora_set(const char* adapter, const char* weight_name, const void* down_dev, size_t down_numel, const void* up_dev,
                     size_t up_numel, mc_dtype dtype, int rank, float factor, hipStream_t stream);
  // the same from the shapes: down_shape [rank, k_in] and up_shape [rows, rank] must share the rank
  mc_status lora_set(const char* adapter, const char* weight_name, const void* down_dev, const int64_t* down_shape, const void* up_dev,
                     const int64_t* up_shape, mc_dtype dtype, float factor, hipStream_t stream);
  // With allow_f32_targets `weight_name` may also be an fp32 matrix (Slot::f32_k): it keeps its own pristine fp32 copy and is
  // rebuilt as base + sum_j ... by launch_lora_merge_f32, with no rounding step.
  // lora_set_delta (allow_f32_targets only): p = base + sum_j scale_j delta_j on an fp32 parameter -- a bias (that of a part of
  // a fused Linear through the slot's offset), a norm weight, a modulation table, an fp32 matrix (there the pairs are merged
  // first and the deltas added to the result) -- by launch_param_delta.  delta_dev: numel fp32 elements, copied.  The rules of
  // a pair: the same (adapter, name) replaces, at most kLoraMaxTerms per parameter, a pristine copy while touched.  A bf16
  // matrix is refused: a full-rank delta is a checkpoint, not an adapter.
  mc_status lora_set_delta(const char* adapter, const char* param_name, const void* delta_dev, size_t numel, mc_dtype dtype,
                           hipStream_t stream);
  // ---- the other kinds of term, on the bf16 parts lora_set takes (an fp32 matrix, a padded or permuted weight: MC_EINVAL
  // naming it).  Operands fp32 or bf16, copied and widened to fp32.  The same (adapter, weight_name) and kind replaces; pairs,
  // Kronecker and Hadamard terms together are at most kLoraMaxTerms per weight.  A part that carries one of these, or a
  // magnitude, is rebuilt by launch_adapter_merge (ops.h states the arithmetic) with an fp32 scratch of the part's size that
  // the apply allocates and frees; a part with live pairs only keeps launch_lora_merge.
  // lora_set_kron: m * kron(w1 [r1, c1], w2 [r2, c2]) with r1 r2 = rows of the part and c1 c2 = in_features.
  mc_status lora_set_kron(const char* adapter, const char* weight_name, const void* w1_dev, const int64_t* w1_shape, const void* w2_dev,
                          const int64_t* w2_shape, mc_dtype dtype, float factor, hipStream_t stream);
  // lora_set_hada: m * (u1 d1) * (u2 d2) element-wise, u1 and u2 [rows, rank] (u_shape), d1 and d2 [rank, in_features] (d_shape)
  mc_status lora_set_hada(const char* adapter, const char* weight_name, const void* u1_dev, const int64_t* u_shape, const void* d1_dev,
                          const int64_t* d_shape, const void* u2_dev, const void* d2_dev, mc_dtype dtype, float factor,
                          hipStream_t stream);
  // lora_set_magnitude: the DoRA magnitude g [rows] of `adapter` on the part: live while the adapter's scale is not 0, the part is
  // then g[r] / |V[r, :]| * V[r, :] with V = W + every live term (other adapters' included).  One magnitude per weight: a second
  // adapter's is MC_EINVAL naming both adapters.
  mc_status lora_set_magnitude(const char* adapter, const char* weight_name, const void* mag_dev, size_t numel, mc_dtype dtype,
                               hipStream_t stream);
  mc_status lora_scale(const char* adapter, float scale);   // a term's multiplier is scale * factor
  mc_status lora_remove(const char* adapter);               // null: every adapter
  // every part whose terms, multipliers or base changed since the last apply: one merge over its rows (a term with multiplier 0
  // is skipped; no live term: the base rows are copied back), then the quantised copy of exactly those rows.  A Linear that no
  // adapter touches any more gives its base copy back.
  // An fp32 parameter that no adapter touches any more gives its copy back likewise.  merged: parameters rebuilt by this call.
  mc_status lora_apply(hipStream_t stream, int* merged = nullptr);
  bool dirty() const { return !lora_dirty.empty(); }
  // adapters known; Linears and fp32 parameters with a pristine copy; bytes of those copies
  void lora_info(int* adapters, int* linears, size_t* base_bytes) const;

  int missing(char* buf, size_t buflen) const;  // count; names, one per line, as far as buf holds them
  bool all_loaded(const char** first_missing) const;
  void release(void* p);  // free one allocation of alloc() (never inside a forward)
  void free_all();

 private:
  mc_status alloc_bytes(void** p, size_t bytes);
  // the quantised copy (q8 / mx) of the rows of `s`, from the bf16 rows just stored in the live weight
  mc_status requantise(const Slot& s, hipStream_t stream);
  // the pristine copy the first term on `s` makes (a Linear's whole bf16 weight | the fp32 parameter's own elements)
  mc_status make_base(Slot& s, hipStream_t stream, bool* made);
  void drop_base(Slot& s);
  mc_status apply_f32(const std::string& name, Slot& s, hipStream_t stream);
  // The slot a term of kind `kind` may go on (`what` names the kind in the error text), or MC_EINVAL naming the weight:
  // KRON, HADA, MAGNITUDE: a plain bf16 part of a Linear | PAIR: that, or with allow_f32_targets an fp32 matrix |
  // DELTA: with allow_f32_targets an fp32 parameter.  A matrix's in_features are a multiple of 8 (bf16) / 4 (fp32): checked
  // here, for a pair by lora_set after its shape checks (one function, host.cpp: check_matrix_k).
  mc_status term_target(const char* what, const char* name, AdapterTerm::Kind kind, Slot** slot);
  // The one way a term gets into `terms`.  Refuses a term beyond kLoraMaxTerms counted ones on the target
  // (AdapterTerm::counts_with), then operands that are neither fp32 nor bf16; allocates t.p[i] of bytes[i] (0: none), makes the
  // base copy of `s`, has `fill` launch the copies into t.p, then replaces the term of the same (adapter, target, kind) in place, freeing its copies, or appends;
  // the adapter is known from then on (scale 1 if new) and the target dirty.  A refusal or failure leaves terms, scales, the
  // dirty set and the base copies as they were.
  template <class Fill>
  mc_status put_term(AdapterTerm t, Slot& s, const char* what, mc_dtype dtype, const size_t (&bytes)[4], Fill fill, hipStream_t stream);
  // KRON, HADA, MAGNITUDE: `n_ops` fp32 or bf16 operands of numel[i] elements, widened into the term's fp32 copies
  mc_status put_widened(AdapterTerm t, Slot& s, const char* what, const void* const* src, const size_t* numel, int n_ops,
                        mc_dtype dtype, hipStream_t stream);
  void release_term(AdapterTerm& t);   // frees whatever copies it holds
  // does a term still need the pristine copy of `s` (a Linear's is shared by its parts)
  bool base_in_use(const Slot& s) const;
  // the launch arrays of `name`: its terms of each kind in list order, a term with multiplier scale * factor == 0 left out; the
  // magnitude is live while its adapter's scale is not 0
  void gather(const std::string& name, TermArrays& a) const;
  // Every adapter's terms, in the order they were set; a replaced term keeps its position.  THE ORDERING INVARIANT: the launch
  // arrays of a merge are the live terms of each kind on the target in this list's order -- pairs, then Kronecker terms, then
  // Hadamard terms, as ops.h states the arithmetic of launch_adapter_merge; on an fp32 parameter the deltas follow the pairs.
  // fp32 sums depend on that order, so merged weights stay bit-identical only while gather() filters this one list by kind.
  std::vector<AdapterTerm> terms;
  std::map<std::string, float> lora_scales;   // adapter -> scale
  std::set<std::string> lora_dirty;           // weight slots to merge again
};

// The element format of an engine's MX Linears, read once by its create call from the options "mx_fp4" / "mx_fp6": MC_EINVAL for
// both at 1; e4m3 when neither is set or the engine has no MX Linears (mx_linears false: fp8_linear < 2).
mc_status latch_mx_format(bool mx_linears, MxFormat* out);
// the K contract of the MX GEMMs on a Linear's in_features (a multiple of 256, at least 512); `what` names the Linear
mc_status check_mx_k(MxFormat fmt, const char* what, int k);

// ---------------------------------------------------------------- workspace
struct Buf {
  size_t off = 0, bytes = 0;
};

// the plan of one caller-owned allocation: named buffers at 256-byte aligned offsets
struct Workspace {
  std::map<std::string, Buf> bufs;
  char* ws = nullptr;
  size_t need = 0;   // bytes planned so far
  size_t bound = 0;  // bytes behind ws

  void add(const char* name, size_t bytes);
  // take over another plan (one made with add() on a Workspace of its own) under the binding of this one: refused, and
  // nothing changed, when memory is bound and the plan does not fit it
  mc_status replan(const Workspace& plan);
  mc_status bind(void* ws_dev, size_t bytes);
  const Buf* find(const std::string& name) const;
  mc_status info(const std::string& name, size_t* offset, size_t* bytes) const;
  template <class T>
  T* get(const char* name) const { return reinterpret_cast<T*>(ptr(name)); }

 private:
  char* ptr(const char* name) const;  // null (and the error text) for a name that is not in the plan
};

// what every entry point that launches needs: a bound workspace and every weight set (`set_workspace` names the call that
// binds one, for the error text)
mc_status check_ready(const Workspace& work, const WeightStore& weights, const char* set_workspace);

// y[:, out] = epilogue(A W[out]^T + b[out]) on bf16 operands: p carries what the epilogue needs, the operands, the shape and
// every pointer advance of a row range come from `l`
hipError_t launch_linear_bf16(const Linear& l, RowRange out, const bf16_t* A, long lda, int M, GemmParams p, int epi, hipStream_t s);

// The keys and values of one attention launch: n_shards blocks of `rows` rows (a multiple of 64; `stride` elements apart), the
// first `valid` of each being keys; the rows up to `rows` are read and masked and must be finite.  skip_shard_p1 = k + 1 leaves
// shard k out.
struct Keys {
  const bf16_t *k, *v;
  long ld, stride;
  int rows, valid, n_shards, skip_shard_p1;
};
// q_rows_pad query rows of Q over one key set -> O.  lse_out: keep the log2-sum-exp of this launch; lse_in: O already holds the
// result over other keys with that log2-sum-exp, merge with it.
hipError_t launch_attention_keys(const bf16_t* Q, long ldq, bf16_t* O, long ldo, int q_rows_pad, int heads, const Keys& keys,
                                 const float* lse_in, float* lse_out, hipStream_t s);

}  // namespace mc
