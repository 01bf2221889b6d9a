// host.h: error text, weight store and workspace plan shared by the engines of this library.
#include "host.h"

#include <cmath>
#include <cstdio>

namespace mc {

namespace {
thread_local char g_err[512] = "";
}

mc_status fail(mc_status s, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return s;
}

const char* last_error() { return g_err; }

// ------------------------------------------------------------------------------------------------ WeightStore
mc_status WeightStore::alloc_bytes(void** p, size_t bytes) {
  void* q = nullptr;
  hipError_t err = hipMalloc(&q, bytes + 256);
  if (err != hipSuccess) return fail(MC_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
  owned.push_back(q);
  *p = q;
  return MC_OK;
}

Slot& WeightStore::add(const std::string& name, void* dst, mc_dtype dt, size_t numel, size_t off) {
  Slot s;
  s.dst = dst; s.dst_dtype = dt; s.numel = numel; s.off = off;
  return slots[name] = s;
}

mc_status WeightStore::add_f32(float*& p, const std::string& name, size_t numel, size_t k_in) {
  MC_TRY(alloc(&p, numel));
  add(name, p, MC_F32, numel).f32_k = k_in;
  return MC_OK;
}

mc_status WeightStore::alloc_linear(Linear& l, size_t n_out, size_t k_in, Quant quant, MxFormat fmt) {
  l.n_out = (int)n_out; l.k_in = (int)k_in;
  l.fmt = fmt;
  MC_TRY(alloc(&l.w, n_out * k_in));
  MC_TRY(alloc(&l.b, n_out));
  if (quant == QUANT_ROW) {
    MC_TRY(alloc(&l.q, n_out * k_in));
    MC_TRY(alloc(&l.q_scale, n_out));
  } else if (quant == QUANT_MX) {
    MC_TRY(alloc(&l.q, n_out * (size_t)mx_row_bytes(fmt, (long)k_in)));
    MC_TRY(alloc(&l.mx, (k_in / 32) * n_out));
  }
  return MC_OK;
}

Slot& WeightStore::add_parts(Linear& l, const std::string& prefix, const std::vector<Part>& parts, size_t row0) {
  const size_t k = l.k_in;
  Slot* last = nullptr;
  for (const Part& part : parts) {
    add(prefix + part.name + ".bias", l.b, MC_F32, part.rows, row0);
    last = &add(prefix + part.name + ".weight", l.w, MC_BF16, part.rows * k, row0 * k);
    last->q8 = l.q; last->q8_scale = l.q_scale; last->q8_k = k; last->mx = l.mx; last->mx_rows = l.n_out;
    last->fmt = l.fmt;
    last->lin = &l;
    row0 += part.rows;
  }
  return *last;
}

mc_status WeightStore::add_linear(Linear& l, const std::string& prefix, const std::vector<Part>& parts, size_t k_in, Quant quant,
                                  MxFormat fmt) {
  size_t n_out = 0;
  for (const Part& part : parts) n_out += part.rows;
  MC_TRY(alloc_linear(l, n_out, k_in, quant, fmt));
  add_parts(l, prefix, parts);
  return MC_OK;
}

mc_status WeightStore::set(const char* name, const void* src_dev, mc_dtype dtype, const int64_t* shape, int ndim,
                           hipStream_t stream) {
  auto it = slots.find(name);
  if (it == slots.end()) return fail(MC_EINVAL, "unknown weight '%s'", name);
  Slot& s = it->second;
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
  if (numel != s.numel) return fail(MC_EINVAL, "weight '%s': %zu elements given, %zu expected", name, numel, s.numel);
  if (s.dst_dtype == MC_F32) {
    if (dtype != MC_F32) return fail(MC_EINVAL, "weight '%s' must be given as fp32", name);
    // a parameter with a base copy keeps the given values there; the live ones follow with the next lora_apply
    float* dst = s.f32_base ? s.f32_base : (float*)s.dst + s.off;
    if (s.f32_base) lora_dirty.insert(name);
    if (s.perm_c > 0) {  // rows (c, pq) -> (pq, c)
      const size_t C = s.perm_c, row = numel / (4 * C);
      for (size_t c = 0; c < C; ++c)
        for (size_t pq = 0; pq < 4; ++pq)
          HIP_TRY(hipMemcpyAsync(dst + (pq * C + c) * row, (const float*)src_dev + (c * 4 + pq) * row, row * 4,
                                 hipMemcpyDeviceToDevice, stream));
    } else {
      HIP_TRY(hipMemcpyAsync(dst, src_dev, numel * 4, hipMemcpyDeviceToDevice, stream));
    }
  } else {
    // a Linear with a base copy keeps the given rows there; the live rows follow with the next lora_apply
    const bool to_base = s.lin && s.lin->w_base;
    bf16_t* dst = (to_base ? s.lin->w_base : (bf16_t*)s.dst) + s.off;
    if (s.pad.rows) {  // [rows, k_in] -> [rows, k_pitch] row pitch (the padding columns stay zero)
      const size_t rows = s.pad.rows, k = s.pad.k_in, pitch = s.pad.k_pitch;
      if (dtype == MC_F32) {
        HIP_TRY(launch_cast_pad_bf16((const float*)src_dev, (long)k, (int)rows, (int)rows, (int)k, dst, (long)pitch, stream));
      } else {
        HIP_TRY(hipMemcpy2DAsync(dst, pitch * 2, src_dev, k * 2, k * 2, rows, hipMemcpyDeviceToDevice, stream));
      }
    } else if (dtype == MC_F32) {
      HIP_TRY(launch_cast_bf16((const float*)src_dev, dst, numel, stream));
    } else {
      HIP_TRY(hipMemcpyAsync(dst, src_dev, numel * 2, hipMemcpyDeviceToDevice, stream));
    }
    if (to_base) lora_dirty.insert(name);
    else MC_TRY(requantise(s, stream));
  }
  s.loaded = true;
  return MC_OK;
}

mc_status WeightStore::requantise(const Slot& s, hipStream_t stream) {
  if (!s.q8) return MC_OK;
  const bf16_t* src = (const bf16_t*)s.dst + s.off;
  const size_t rows = s.numel / s.q8_k, row0 = s.off / s.q8_k;
  if (s.mx) {  // MX: the packed rows are relative to the block scales, not to a row scale (s.off is a whole number of rows)
    const long row_bytes = mx_row_bytes(s.fmt, (long)s.q8_k);
    HIP_TRY(launch_quantize_rows_mx(s.fmt, src, nullptr, (long)s.q8_k, (int)rows, (int)s.q8_k, s.q8 + row0 * row_bytes, row_bytes,
                                    s.mx + row0, (long)s.mx_rows, stream));
  } else {
    HIP_TRY(launch_quantize_rows_fp8(src, nullptr, (long)s.q8_k, (int)rows, (int)s.q8_k, s.q8 + s.off, (long)s.q8_k,
                                     s.q8_scale + row0, stream));
  }
  return MC_OK;
}

// ------------------------------------------------------------------------------------------------ the MX format latch
mc_status latch_mx_format(bool mx_linears, MxFormat* out) {
  if (g_mx_fp4 != 0 && g_mx_fp6 != 0)
    return fail(MC_EINVAL, "the options \"mx_fp4\" and \"mx_fp6\" are both 1: an engine's MX Linears hold one element format, set one of them");
  *out = !mx_linears ? MX_E4M3 : g_mx_fp4 != 0 ? MX_E2M1 : g_mx_fp6 != 0 ? MX_E2M3 : MX_E4M3;
  return MC_OK;
}

mc_status check_mx_k(MxFormat fmt, const char* what, int k) {
  if ((k % 256) == 0 && k >= 512) return MC_OK;
  return fail(MC_EINVAL, "%s: %s: %d input features are no multiple of 256 >= 512 (the K contract of the %s GEMM)", mx_info(fmt).option,
              what, k, mx_info(fmt).name);
}

// ------------------------------------------------------------------------------------------------ LoRA adapters
mc_status WeightStore::make_base(Slot& s, hipStream_t stream, bool* made) {
  *made = false;
  if (s.lin ? s.lin->w_base != nullptr : s.f32_base != nullptr) return MC_OK;
  hipError_t err;
  if (s.lin) {
    Linear& l = *s.lin;
    const size_t n = (size_t)l.n_out * l.k_in;
    MC_TRY(alloc(&l.w_base, n));
    err = hipMemcpyAsync(l.w_base, l.w, n * 2, hipMemcpyDeviceToDevice, stream);
  } else {
    MC_TRY(alloc(&s.f32_base, s.numel));
    err = hipMemcpyAsync(s.f32_base, (const float*)s.dst + s.off, s.numel * 4, hipMemcpyDeviceToDevice, stream);
  }
  if (err != hipSuccess) {
    drop_base(s);
    return fail(MC_EHIP, "LoRA: the base copy failed: %s", hipGetErrorString(err));
  }
  *made = true;
  return MC_OK;
}

void WeightStore::drop_base(Slot& s) {   // hipFree waits for the launches that may still read the copy
  if (s.lin) { release(s.lin->w_base); s.lin->w_base = nullptr; }
  else { release(s.f32_base); s.f32_base = nullptr; }
}

bool WeightStore::base_in_use(const Slot& s) const {
  for (const AdapterTerm& t : terms) {
    const Slot& o = slots.at(t.target);
    if (s.lin ? o.lin == s.lin : &o == &s) return true;
  }
  return false;
}

void WeightStore::release_term(AdapterTerm& t) {
  for (void*& q : t.p) {
    if (q) release(q);
    q = nullptr;
  }
}

// in_features of a matrix that takes terms: a part of a Linear, or an fp32 matrix
static size_t matrix_k(const Slot& s) { return s.lin ? (size_t)s.lin->k_in : s.f32_k; }
// ... which are whole 16-byte vectors of the merge kernels: 8 bf16, 4 fp32 elements
static mc_status check_matrix_k(const char* what, const char* name, const Slot& s) {
  const int step = s.lin ? 8 : 4;
  if ((matrix_k(s) % step) == 0) return MC_OK;
  return fail(MC_EINVAL, "%s '%s': in_features %zu is no multiple of %d", what, name, matrix_k(s), step);
}

mc_status WeightStore::term_target(const char* what, const char* name, AdapterTerm::Kind kind, Slot** slot) {
  auto it = slots.find(name);
  if (it == slots.end()) return fail(MC_EINVAL, "%s: unknown weight '%s'", what, name);
  Slot& s = it->second;
  *slot = &s;
  if (kind == AdapterTerm::DELTA) {
    if (s.dst_dtype != MC_F32)
      return fail(MC_EINVAL, "%s: '%s' is a bf16 matrix and takes low-rank pairs only (a full-rank delta is a checkpoint, not an adapter)",
                  what, name);
    if (!allow_f32_targets || s.perm_c || s.fixed) return fail(MC_EINVAL, "%s: '%s' takes no delta in this engine", what, name);
    return MC_OK;
  }
  const bool part = s.lin && s.dst_dtype == MC_BF16 && !s.pad.rows && !s.perm_c && !s.fixed;
  const bool f32_matrix = kind == AdapterTerm::PAIR && allow_f32_targets && s.dst_dtype == MC_F32 && s.f32_k > 0 && !s.perm_c && !s.fixed;
  if (!part && !f32_matrix)
    return fail(MC_EINVAL, "%s: '%s' is no plain bf16 part of a Linear (an fp32, padded or permuted weight takes %s)", what, name,
                kind == AdapterTerm::PAIR ? "no adapter" : "low-rank pairs at most");
  return kind == AdapterTerm::PAIR ? MC_OK : check_matrix_k(what, name, s);   // a pair: after its shape checks (lora_set)
}

template <class Fill>
mc_status WeightStore::put_term(AdapterTerm t, Slot& s, const char* what, mc_dtype dtype, const size_t (&bytes)[4], Fill fill,
                                hipStream_t stream) {
  size_t at = terms.size(), counted = 0;
  for (size_t i = 0; i < terms.size(); ++i) {
    if (terms[i].target != t.target) continue;
    if (terms[i].adapter == t.adapter && terms[i].kind == t.kind) at = i;
    else if (terms[i].counts_with(t.kind)) ++counted;
  }
  if (counted + 1 > (size_t)kLoraMaxTerms)
    return fail(MC_EINVAL, "%s '%s': more than %d adapters on one weight", what, t.target.c_str(), kLoraMaxTerms);
  if (dtype != MC_F32 && dtype != MC_BF16) return fail(MC_EINVAL, "adapter '%s' on '%s': operands are fp32 or bf16", t.adapter.c_str(), t.target.c_str());
  for (int i = 0; i < 4; ++i)
    if (bytes[i] > 0)
      if (mc_status st = alloc_bytes(&t.p[i], bytes[i])) { release_term(t); return st; }
  bool new_base = false;   // the first term on this Linear (this fp32 parameter): its pristine copy
  if (mc_status st = make_base(s, stream, &new_base)) { release_term(t); return st; }
  const hipError_t err = fill(t);
  if (err != hipSuccess) {
    release_term(t);
    if (new_base) drop_base(s);
    return fail(MC_EHIP, "%s '%s': %s", what, t.target.c_str(), hipGetErrorString(err));
  }
  if (at < terms.size()) {  // replaced, in its place: the old copies go (hipFree waits for a merge that may still read them)
    release_term(terms[at]);
    terms[at] = t;
  } else {
    terms.push_back(t);
  }
  lora_scales.emplace(t.adapter, 1.f);
  lora_dirty.insert(t.target);
  return MC_OK;
}

mc_status WeightStore::lora_set(const char* adapter, const char* weight_name, const void* down_dev, const int64_t* down_shape,
                                const void* up_dev, const int64_t* up_shape, mc_dtype dtype, float factor, hipStream_t stream) {
  if (!adapter || !weight_name || !down_dev || !down_shape || !up_dev || !up_shape) return fail(MC_EINVAL, "null argument");
  if (down_shape[0] <= 0 || down_shape[0] > (1 << 20) || down_shape[1] <= 0 || up_shape[0] <= 0 || up_shape[1] != down_shape[0])
    return fail(MC_EINVAL, "LoRA '%s': down [%lld, %lld] and up [%lld, %lld] share no rank", weight_name, (long long)down_shape[0],
                (long long)down_shape[1], (long long)up_shape[0], (long long)up_shape[1]);
  return lora_set(adapter, weight_name, down_dev, (size_t)down_shape[0] * down_shape[1], up_dev, (size_t)up_shape[0] * up_shape[1], dtype,
                  (int)down_shape[0], factor, stream);
}

mc_status WeightStore::lora_set(const char* adapter, const char* weight_name, const void* down_dev, size_t down_numel,
                                const void* up_dev, size_t up_numel, mc_dtype dtype, int rank, float factor, hipStream_t stream) {
  Slot* s = nullptr;
  MC_TRY(term_target("LoRA", weight_name, AdapterTerm::PAIR, &s));
  if (dtype != MC_F32 && dtype != MC_BF16) return fail(MC_EINVAL, "LoRA '%s': down / up are fp32 or bf16", weight_name);
  const size_t k = matrix_k(*s), rows = s->numel / k;
  if (rank <= 0) return fail(MC_EINVAL, "LoRA '%s': rank %d", weight_name, rank);
  if (down_numel != (size_t)rank * k || up_numel != rows * (size_t)rank)
    return fail(MC_EINVAL, "LoRA '%s': down has %zu elements, up %zu; rank %d wants [%d, %zu] = %zu and [%zu, %d] = %zu", weight_name,
                down_numel, up_numel, rank, rank, k, (size_t)rank * k, rows, rank, rows * (size_t)rank);
  MC_TRY(check_matrix_k("LoRA", weight_name, *s));
  AdapterTerm t;
  t.adapter = adapter; t.target = weight_name; t.kind = AdapterTerm::PAIR; t.factor = factor;
  t.rank = rank; t.rank_pad = (int)align_up(rank, kLoraRankStep);
  const size_t bytes[4] = {lora_packed_elems(rows, t.rank_pad) * sizeof(bf16_t), lora_packed_elems(k, t.rank_pad) * sizeof(bf16_t), 0, 0};
  return put_term(t, *s, "LoRA", dtype, bytes, [&](const AdapterTerm& n) {
    hipError_t err = launch_lora_pack(up_dev, dtype == MC_F32, rank, 1, (int)rows, rank, n.rank_pad, (bf16_t*)n.p[0], stream);
    if (err == hipSuccess) err = launch_lora_pack(down_dev, dtype == MC_F32, 1, (long)k, (int)k, rank, n.rank_pad, (bf16_t*)n.p[1], stream);
    return err;
  }, stream);
}

mc_status WeightStore::lora_set_delta(const char* adapter, const char* param_name, const void* delta_dev, size_t numel, mc_dtype dtype,
                                      hipStream_t stream) {
  if (!adapter || !param_name || !delta_dev) return fail(MC_EINVAL, "null argument");
  Slot* s = nullptr;
  MC_TRY(term_target("LoRA", param_name, AdapterTerm::DELTA, &s));
  if (dtype != MC_F32) return fail(MC_EINVAL, "LoRA '%s': a delta must be given as fp32", param_name);
  if (numel != s->numel) return fail(MC_EINVAL, "LoRA '%s': a delta of %zu elements, %zu expected", param_name, numel, s->numel);
  AdapterTerm t;
  t.adapter = adapter; t.target = param_name; t.kind = AdapterTerm::DELTA;
  const size_t bytes[4] = {numel * sizeof(float), 0, 0, 0};
  return put_term(t, *s, "LoRA", dtype, bytes, [&](const AdapterTerm& n) {
    return hipMemcpyAsync(n.p[0], delta_dev, numel * sizeof(float), hipMemcpyDeviceToDevice, stream);
  }, stream);
}

// ---- Kronecker and Hadamard terms, DoRA magnitudes
mc_status WeightStore::put_widened(AdapterTerm t, Slot& s, const char* what, const void* const* src, const size_t* numel, int n_ops,
                                   mc_dtype dtype, hipStream_t stream) {
  size_t bytes[4] = {0, 0, 0, 0};
  for (int i = 0; i < n_ops; ++i) bytes[i] = numel[i] * sizeof(float);
  return put_term(t, s, what, dtype, bytes, [&](const AdapterTerm& n) {
    hipError_t err = hipSuccess;
    for (int i = 0; i < n_ops && err == hipSuccess; ++i) err = launch_widen_f32(src[i], dtype == MC_F32, (float*)n.p[i], numel[i], stream);
    return err;
  }, stream);
}

mc_status WeightStore::lora_set_kron(const char* adapter, const char* weight_name, const void* w1_dev, const int64_t* w1_shape,
                                     const void* w2_dev, const int64_t* w2_shape, mc_dtype dtype, float factor, hipStream_t stream) {
  if (!adapter || !weight_name || !w1_dev || !w1_shape || !w2_dev || !w2_shape) return fail(MC_EINVAL, "null argument");
  Slot* s = nullptr;
  MC_TRY(term_target("LoKr", weight_name, AdapterTerm::KRON, &s));
  const size_t k = matrix_k(*s), rows = s->numel / k;
  const int64_t lim = 1 << 30;
  for (const int64_t v : {w1_shape[0], w1_shape[1], w2_shape[0], w2_shape[1]})
    if (v < 1 || v > lim)
      return fail(MC_EINVAL, "LoKr '%s': factor shapes [%lld, %lld] and [%lld, %lld]", weight_name, (long long)w1_shape[0],
                  (long long)w1_shape[1], (long long)w2_shape[0], (long long)w2_shape[1]);
  AdapterTerm t;
  t.adapter = adapter; t.target = weight_name; t.kind = AdapterTerm::KRON; t.factor = factor;
  t.r1 = (int)w1_shape[0]; t.c1 = (int)w1_shape[1]; t.r2 = (int)w2_shape[0]; t.c2 = (int)w2_shape[1];
  if ((size_t)t.r1 * (size_t)t.r2 != rows || (size_t)t.c1 * (size_t)t.c2 != k)
    return fail(MC_EINVAL, "LoKr '%s': [%d, %d] (x) [%d, %d] is no factorisation of [%zu, %zu]", weight_name, t.r1, t.c1, t.r2, t.c2, rows, k);
  const void* src[2] = {w1_dev, w2_dev};
  const size_t numel[2] = {(size_t)t.r1 * t.c1, (size_t)t.r2 * t.c2};
  return put_widened(t, *s, "LoKr", src, numel, 2, dtype, stream);
}

mc_status WeightStore::lora_set_hada(const char* adapter, const char* weight_name, const void* u1_dev, const int64_t* u_shape,
                                     const void* d1_dev, const int64_t* d_shape, const void* u2_dev, const void* d2_dev, mc_dtype dtype,
                                     float factor, hipStream_t stream) {
  if (!adapter || !weight_name || !u1_dev || !u_shape || !d1_dev || !d_shape || !u2_dev || !d2_dev) return fail(MC_EINVAL, "null argument");
  Slot* s = nullptr;
  MC_TRY(term_target("LoHa", weight_name, AdapterTerm::HADA, &s));
  const size_t k = matrix_k(*s), rows = s->numel / k;
  if (u_shape[1] < 1 || u_shape[1] > (1 << 20) || d_shape[0] != u_shape[1])
    return fail(MC_EINVAL, "LoHa '%s': [%lld, %lld] and [%lld, %lld] share no rank", weight_name, (long long)u_shape[0],
                (long long)u_shape[1], (long long)d_shape[0], (long long)d_shape[1]);
  if (u_shape[0] != (int64_t)rows || d_shape[1] != (int64_t)k)
    return fail(MC_EINVAL, "LoHa '%s': factors for a [%lld, %lld] weight, the weight is [%zu, %zu]", weight_name, (long long)u_shape[0],
                (long long)d_shape[1], rows, k);
  AdapterTerm t;
  t.adapter = adapter; t.target = weight_name; t.kind = AdapterTerm::HADA; t.factor = factor; t.rank = (int)u_shape[1];
  const void* src[4] = {u1_dev, d1_dev, u2_dev, d2_dev};
  const size_t up = rows * (size_t)t.rank, down = (size_t)t.rank * k;
  const size_t numel[4] = {up, down, up, down};
  return put_widened(t, *s, "LoHa", src, numel, 4, dtype, stream);
}

mc_status WeightStore::lora_set_magnitude(const char* adapter, const char* weight_name, const void* mag_dev, size_t numel, mc_dtype dtype,
                                          hipStream_t stream) {
  if (!adapter || !weight_name || !mag_dev) return fail(MC_EINVAL, "null argument");
  Slot* s = nullptr;
  MC_TRY(term_target("DoRA", weight_name, AdapterTerm::MAGNITUDE, &s));
  const size_t rows = s->numel / matrix_k(*s);
  if (numel != rows) return fail(MC_EINVAL, "DoRA '%s': a magnitude of %zu elements, %zu output rows", weight_name, numel, rows);
  for (const AdapterTerm& o : terms)
    if (o.kind == AdapterTerm::MAGNITUDE && o.target == weight_name && o.adapter != adapter)
      return fail(MC_EINVAL, "DoRA '%s': adapter '%s' brings a magnitude, adapter '%s' already has one on this weight (one magnitude "
                             "normalises a weight)", weight_name, adapter, o.adapter.c_str());
  AdapterTerm t;
  t.adapter = adapter; t.target = weight_name; t.kind = AdapterTerm::MAGNITUDE;
  const void* src[1] = {mag_dev};
  return put_widened(t, *s, "DoRA", src, &numel, 1, dtype, stream);
}

mc_status WeightStore::lora_scale(const char* adapter, float scale) {
  if (!adapter) return fail(MC_EINVAL, "null argument");
  auto it = lora_scales.find(adapter);
  if (it == lora_scales.end()) return fail(MC_EINVAL, "LoRA: unknown adapter '%s'", adapter);
  if (it->second == scale) return MC_OK;
  it->second = scale;
  for (const AdapterTerm& t : terms)
    if (t.adapter == adapter) lora_dirty.insert(t.target);
  return MC_OK;
}

mc_status WeightStore::lora_remove(const char* adapter) {
  if (adapter && !lora_scales.count(adapter)) return fail(MC_EINVAL, "LoRA: unknown adapter '%s'", adapter);
  std::vector<AdapterTerm> kept;
  for (AdapterTerm& t : terms) {
    if (adapter && t.adapter != adapter) { kept.push_back(t); continue; }
    lora_dirty.insert(t.target);
    release_term(t);
  }
  terms.swap(kept);
  if (adapter) lora_scales.erase(adapter);
  else lora_scales.clear();
  return MC_OK;
}

// ---- apply
struct TermArrays {
  LoraTerm pairs[kLoraMaxTerms];
  KronTerm krons[kLoraMaxTerms];
  HadaTerm hadas[kLoraMaxTerms];
  const float* deltas[kLoraMaxTerms];
  float delta_scales[kLoraMaxTerms];
  int n = 0, nk = 0, nh = 0, nd = 0;
  const float* magnitude = nullptr;   // at most one per weight (lora_set_magnitude)
};

void WeightStore::gather(const std::string& name, TermArrays& a) const {
  for (const AdapterTerm& t : terms) {
    if (t.target != name) continue;
    const float scale = lora_scales.at(t.adapter), m = scale * t.factor;
    if (t.kind == AdapterTerm::MAGNITUDE) {
      if (scale != 0.f) a.magnitude = t.f32(0);
    } else if (m == 0.f) {
      continue;
    } else if (t.kind == AdapterTerm::PAIR) {
      a.pairs[a.n++] = LoraTerm{(const bf16_t*)t.p[0], (const bf16_t*)t.p[1], t.rank_pad, m};
    } else if (t.kind == AdapterTerm::DELTA) {
      a.deltas[a.nd] = t.f32(0);
      a.delta_scales[a.nd++] = m;
    } else if (t.kind == AdapterTerm::KRON) {
      a.krons[a.nk++] = KronTerm{t.f32(0), t.f32(1), t.r1, t.c1, t.r2, t.c2, m};
    } else {
      a.hadas[a.nh++] = HadaTerm{t.f32(0), t.f32(1), t.f32(2), t.f32(3), t.rank, m};
    }
  }
}

// an fp32 parameter: the pairs of a matrix first (base -> live), then the deltas (base, or that result, -> live)
mc_status WeightStore::apply_f32(const std::string& name, Slot& s, hipStream_t stream) {
  float* live = (float*)s.dst + s.off;
  if (!s.f32_base) return MC_OK;   // set before its first term and never touched: live is the value
  TermArrays a;
  gather(name, a);
  hipError_t err = hipSuccess;
  if (a.n > 0) {
    const size_t k = s.f32_k;
    err = launch_lora_merge_f32(s.f32_base, (long)k, live, (long)k, (int)(s.numel / k), (int)k, a.pairs, a.n, stream);
    if (err == hipSuccess && a.nd > 0) err = launch_param_delta(live, live, s.numel, a.deltas, a.delta_scales, a.nd, stream);
  } else if (a.nd > 0) {
    err = launch_param_delta(s.f32_base, live, s.numel, a.deltas, a.delta_scales, a.nd, stream);
  } else {
    err = hipMemcpyAsync(live, s.f32_base, s.numel * 4, hipMemcpyDeviceToDevice, stream);
  }
  if (err != hipSuccess) return fail(MC_EHIP, "LoRA merge of '%s': %s", name.c_str(), hipGetErrorString(err));
  if (!base_in_use(s)) drop_base(s);   // no adapter left: live is the base again, bit for bit
  return MC_OK;
}

mc_status WeightStore::lora_apply(hipStream_t stream, int* merged) {
  std::vector<Slot*> touched;
  if (merged) *merged = 0;
  while (!lora_dirty.empty()) {
    const std::string name = *lora_dirty.begin();
    Slot& s = slots.at(name);
    if (merged) ++*merged;
    if (!s.lin) {
      MC_TRY(apply_f32(name, s, stream));
      lora_dirty.erase(name);
      continue;
    }
    Linear& l = *s.lin;
    const size_t k = l.k_in, rows = s.numel / k;
    TermArrays a;
    gather(name, a);
    if (a.nk + a.nh > 0 || a.magnitude) {  // the general merge, over an fp32 image of the part that lives for this launch only
      float* scratch = nullptr;
      hipError_t err = hipMalloc((void**)&scratch, rows * k * sizeof(float));
      if (err != hipSuccess) return fail(MC_ENOMEM, "adapter merge of '%s': hipMalloc(%zu) failed: %s", name.c_str(), rows * k * sizeof(float), hipGetErrorString(err));
      err = launch_adapter_merge(l.w_base + s.off, (long)k, l.w + s.off, (long)k, (int)rows, (int)k, a.pairs, a.n, a.krons, a.nk, a.hadas,
                                 a.nh, a.magnitude, scratch, stream);
      if (err == hipSuccess) err = hipStreamSynchronize(stream);
      (void)hipFree(scratch);
      if (err != hipSuccess) return fail(MC_EHIP, "adapter merge of '%s': %s", name.c_str(), hipGetErrorString(err));
    } else if (a.n == 0) {
      HIP_TRY(hipMemcpyAsync(l.w + s.off, l.w_base + s.off, s.numel * 2, hipMemcpyDeviceToDevice, stream));
    } else {
      hipError_t err = launch_lora_merge(l.w_base + s.off, (long)k, l.w + s.off, (long)k, (int)rows, (int)k, a.pairs, a.n, stream);
      if (err != hipSuccess) return fail(MC_EHIP, "LoRA merge of '%s': %s", name.c_str(), hipGetErrorString(err));
    }
    MC_TRY(requantise(s, stream));
    touched.push_back(&s);
    lora_dirty.erase(name);
  }
  for (Slot* s : touched)   // no adapter left on any part of the Linear: w is the base again, bit for bit
    if (s->lin->w_base && !base_in_use(*s)) drop_base(*s);   // hipFree waits for the copies above
  return MC_OK;
}

void WeightStore::lora_info(int* adapters, int* linears, size_t* base_bytes) const {
  std::set<const Linear*> seen;
  size_t bytes = 0;
  int n_f32 = 0;
  for (auto& kv : slots) {
    const Linear* l = kv.second.lin;
    if (l && l->w_base && seen.insert(l).second) bytes += (size_t)l->n_out * l->k_in * 2;
    if (kv.second.f32_base) { ++n_f32; bytes += kv.second.numel * 4; }
  }
  if (adapters) *adapters = (int)lora_scales.size();
  if (linears) *linears = (int)seen.size() + n_f32;
  if (base_bytes) *base_bytes = bytes;
}

int WeightStore::missing(char* buf, size_t buflen) const {
  int n = 0;
  size_t pos = 0;
  if (buf && buflen) buf[0] = 0;
  for (auto& kv : slots) {
    if (kv.second.loaded) continue;
    ++n;
    if (buf && pos + kv.first.size() + 2 < buflen) {
      memcpy(buf + pos, kv.first.c_str(), kv.first.size());
      pos += kv.first.size();
      buf[pos++] = '\n';
      buf[pos] = 0;
    }
  }
  return n;
}

bool WeightStore::all_loaded(const char** first_missing) const {
  for (auto& kv : slots)
    if (!kv.second.loaded) {
      if (first_missing) *first_missing = kv.first.c_str();
      return false;
    }
  return true;
}

void WeightStore::release(void* p) {
  for (size_t i = 0; i < owned.size(); ++i)
    if (owned[i] == p) {
      (void)hipFree(p);
      owned.erase(owned.begin() + i);
      return;
    }
}

void WeightStore::free_all() {
  for (void* p : owned) (void)hipFree(p);
  owned.clear();
}

// ------------------------------------------------------------------------------------------------ Workspace
void Workspace::add(const char* name, size_t bytes) {
  Buf b;
  b.off = need; b.bytes = bytes;
  bufs[name] = b;
  need = align_up(need + bytes, 256);
}

mc_status Workspace::replan(const Workspace& plan) {
  if (ws && plan.need > bound)
    return fail(MC_EINVAL, "the new plan needs a workspace of %zu bytes, %zu bytes are bound", plan.need, bound);
  bufs = plan.bufs;
  need = plan.need;
  return MC_OK;
}

mc_status Workspace::bind(void* ws_dev, size_t bytes) {
  if (!ws_dev) return fail(MC_EINVAL, "null argument");
  if (bytes < need) return fail(MC_EINVAL, "workspace too small: %zu < %zu", bytes, need);
  if (((uintptr_t)ws_dev) & 255) return fail(MC_EINVAL, "workspace must be 256-byte aligned");
  ws = (char*)ws_dev;
  bound = bytes;
  return MC_OK;
}

const Buf* Workspace::find(const std::string& name) const {
  auto it = bufs.find(name);
  return it == bufs.end() ? nullptr : &it->second;
}

mc_status Workspace::info(const std::string& name, size_t* offset, size_t* bytes) const {
  const Buf* b = find(name);
  if (!b) return fail(MC_EINVAL, "unknown buffer '%s'", name.c_str());
  if (offset) *offset = b->off;
  if (bytes) *bytes = b->bytes;
  return MC_OK;
}

char* Workspace::ptr(const char* name) const {
  const Buf* b = find(name);
  if (!b) {
    fail(MC_EINVAL, "unknown buffer '%s'", name);
    return nullptr;
  }
  return ws + b->off;
}

// ------------------------------------------------------------------------------------------------ shared by the engines
mc_status check_ready(const Workspace& work, const WeightStore& weights, const char* set_workspace) {
  if (!work.ws) return fail(MC_ESTATE, "workspace not set (%s)", set_workspace);
  const char* name = nullptr;
  if (!weights.all_loaded(&name)) return fail(MC_ESTATE, "weight '%s' was never set", name);
  return MC_OK;
}

hipError_t launch_linear_bf16(const Linear& l, RowRange out, const bf16_t* A, long lda, int M, GemmParams p, int epi, hipStream_t s) {
  p.A = A; p.lda = lda; p.M = M; p.N = out.count; p.K = l.k_in;
  p.W = l.w + (size_t)out.first * l.k_in; p.ldw = l.k_in; p.bias = l.b + out.first;
  return launch_gemm_bf16(p, epi, s);
}

hipError_t launch_attention_keys(const bf16_t* Q, long ldq, bf16_t* O, long ldo, int q_rows_pad, int heads, const Keys& keys,
                                 const float* lse_in, float* lse_out, hipStream_t s) {
  AttnParams a;
  memset(&a, 0, sizeof(a));
  a.Q = Q; a.ldq = ldq; a.O = O; a.ldo = ldo;
  a.K = keys.k; a.ldk = keys.ld; a.k_shard_stride = keys.stride;
  a.V = keys.v; a.ldv = keys.ld; a.v_shard_stride = keys.stride;
  a.Lq_pad = q_rows_pad; a.n_heads = heads; a.scale = 1.0f / std::sqrt(128.0f);   // head_dim is fixed at 128
  a.shard_rows = keys.rows; a.shard_valid = keys.valid; a.n_shards = keys.n_shards; a.skip_shard_p1 = keys.skip_shard_p1;
  a.lse_in = lse_in; a.lse_out = lse_out;
  return launch_attention(a, s);
}

}  // namespace mc
