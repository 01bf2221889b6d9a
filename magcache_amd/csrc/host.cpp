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
mc_status WeightStore::lora_set(const char* adapter, const char* weight_name, const void* down_dev, size_t down_numel,
                                const void* up_dev, size_t up_numel, mc_dtype dtype, int rank, float factor, hipStream_t stream) {
  auto it = slots.find(weight_name);
  if (it == slots.end()) return fail(MC_EINVAL, "LoRA: unknown weight '%s'", weight_name);
  Slot& s = it->second;
  const bool f32_matrix = allow_f32_targets && s.dst_dtype == MC_F32 && s.f32_k > 0 && !s.perm_c && !s.fixed;
  if (!f32_matrix && (!s.lin || s.dst_dtype != MC_BF16 || s.pad.rows || s.perm_c || s.fixed))
    return fail(MC_EINVAL, "LoRA: '%s' is no plain bf16 part of a Linear (an fp32, padded or permuted weight takes no adapter)",
                weight_name);
  if (dtype != MC_F32 && dtype != MC_BF16) return fail(MC_EINVAL, "LoRA '%s': down / up are fp32 or bf16", weight_name);
  const size_t k = f32_matrix ? s.f32_k : (size_t)s.lin->k_in, rows = s.numel / k;
  if (rank <= 0) return fail(MC_EINVAL, "LoRA '%s': rank %d", weight_name, rank);
  if (down_numel != (size_t)rank * k || up_numel != rows * (size_t)rank)
    return fail(MC_EINVAL, "LoRA '%s': down has %zu elements, up %zu; rank %d wants [%d, %zu] = %zu and [%zu, %d] = %zu", weight_name,
                down_numel, up_numel, rank, rank, k, (size_t)rank * k, rows, rank, rows * (size_t)rank);
  if ((k % (f32_matrix ? 4 : 8)) != 0)
    return fail(MC_EINVAL, "LoRA '%s': in_features %zu is no multiple of %d", weight_name, k, f32_matrix ? 4 : 8);
  size_t at = lora.size();
  for (size_t i = 0; i < lora.size(); ++i)
    if (lora[i].target == weight_name && lora[i].adapter == adapter) at = i;
  if (other_terms(adapter, weight_name, -1) + 1 > (size_t)kLoraMaxTerms)
    return fail(MC_EINVAL, "LoRA '%s': more than %d adapters on one weight", weight_name, kLoraMaxTerms);
  const int rank_pad = (int)align_up(rank, kLoraRankStep);
  LoraPair p;
  p.adapter = adapter; p.target = weight_name; p.rank_pad = rank_pad; p.factor = factor;
  MC_TRY(alloc(&p.up, lora_packed_elems(rows, rank_pad)));
  if (mc_status st = alloc(&p.down_t, lora_packed_elems(k, rank_pad))) { release(p.up); return st; }
  bool new_base = false;   // the first adapter on this Linear (this fp32 matrix): its pristine copy
  if (mc_status st = make_base(s, stream, &new_base)) { release(p.up); release(p.down_t); return st; }
  hipError_t err = launch_lora_pack(up_dev, dtype == MC_F32, rank, 1, (int)rows, rank, rank_pad, p.up, stream);
  if (err == hipSuccess) err = launch_lora_pack(down_dev, dtype == MC_F32, 1, (long)k, (int)k, rank, rank_pad, p.down_t, stream);
  if (err != hipSuccess) {
    release(p.up); release(p.down_t);
    if (new_base) drop_base(s);
    return fail(MC_EHIP, "LoRA '%s': %s", weight_name, hipGetErrorString(err));
  }
  if (at < lora.size()) {  // replaced: the old pair's copies go (hipFree waits for a merge that may still read them)
    release(lora[at].up); release(lora[at].down_t);
    lora[at] = p;
  } else {
    lora.push_back(p);
  }
  lora_scales.emplace(adapter, 1.f);
  lora_dirty.insert(weight_name);
  return MC_OK;
}

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

// ---- Kronecker and Hadamard terms, DoRA magnitudes
size_t WeightStore::other_terms(const char* adapter, const char* weight_name, int kind) const {
  size_t n = 0;
  for (const LoraPair& p : lora)
    if (p.target == weight_name && !(kind < 0 && p.adapter == adapter)) ++n;
  for (const AdapterExtra& x : extras)
    if (x.target == weight_name && x.kind != AdapterExtra::MAGNITUDE && !(kind == (int)x.kind && x.adapter == adapter)) ++n;
  return n;
}

mc_status WeightStore::extra_target(const char* what, const char* weight_name, Slot** slot) {
  auto it = slots.find(weight_name);
  if (it == slots.end()) return fail(MC_EINVAL, "%s: unknown weight '%s'", what, weight_name);
  Slot& s = it->second;
  if (!s.lin || s.dst_dtype != MC_BF16 || s.pad.rows || s.perm_c || s.fixed)
    return fail(MC_EINVAL, "%s: '%s' is no plain bf16 part of a Linear (an fp32, padded or permuted weight takes low-rank pairs at most)",
                what, weight_name);
  if ((s.lin->k_in % 8) != 0) return fail(MC_EINVAL, "%s '%s': in_features %d is no multiple of 8", what, weight_name, s.lin->k_in);
  *slot = &s;
  return MC_OK;
}

void WeightStore::release_extra(AdapterExtra& x) {
  for (float*& q : x.p) {
    if (q) release(q);
    q = nullptr;
  }
}

mc_status WeightStore::store_extra(AdapterExtra x, Slot& s, const void* const* src, const size_t* numel, int n_ops, mc_dtype dtype,
                                   hipStream_t stream) {
  if (dtype != MC_F32 && dtype != MC_BF16) return fail(MC_EINVAL, "adapter '%s' on '%s': operands are fp32 or bf16", x.adapter.c_str(), x.target.c_str());
  for (int i = 0; i < n_ops; ++i)
    if (mc_status st = alloc(&x.p[i], numel[i])) { release_extra(x); return st; }
  bool new_base = false;
  if (mc_status st = make_base(s, stream, &new_base)) { release_extra(x); return st; }
  hipError_t err = hipSuccess;
  for (int i = 0; i < n_ops && err == hipSuccess; ++i) err = launch_widen_f32(src[i], dtype == MC_F32, x.p[i], numel[i], stream);
  if (err != hipSuccess) {
    release_extra(x);
    if (new_base) drop_base(s);
    return fail(MC_EHIP, "adapter '%s' on '%s': %s", x.adapter.c_str(), x.target.c_str(), hipGetErrorString(err));
  }
  size_t at = extras.size();
  for (size_t i = 0; i < extras.size(); ++i)
    if (extras[i].target == x.target && extras[i].adapter == x.adapter && extras[i].kind == x.kind) at = i;
  if (at < extras.size()) {  // replaced: the old copies go (hipFree waits for a merge that may still read them)
    release_extra(extras[at]);
    extras[at] = x;
  } else {
    extras.push_back(x);
  }
  lora_scales.emplace(x.adapter, 1.f);
  lora_dirty.insert(x.target);
  return MC_OK;
}

mc_status WeightStore::lora_set_kron(const char* adapter, const char* weight_name, const void* w1_dev, const int64_t* w1_shape,
                                     const void* w2_dev, const int64_t* w2_shape, mc_dtype dtype, float factor, hipStream_t stream) {
  if (!adapter || !weight_name || !w1_dev || !w1_shape || !w2_dev || !w2_shape) return fail(MC_EINVAL, "null argument");
  Slot* s = nullptr;
  MC_TRY(extra_target("LoKr", weight_name, &s));
  const size_t k = (size_t)s->lin->k_in, rows = s->numel / k;
  const int64_t lim = 1 << 30;
  for (const int64_t v : {w1_shape[0], w1_shape[1], w2_shape[0], w2_shape[1]})
    if (v < 1 || v > lim)
      return fail(MC_EINVAL, "LoKr '%s': factor shapes [%lld, %lld] and [%lld, %lld]", weight_name, (long long)w1_shape[0],
                  (long long)w1_shape[1], (long long)w2_shape[0], (long long)w2_shape[1]);
  const int r1 = (int)w1_shape[0], c1 = (int)w1_shape[1], r2 = (int)w2_shape[0], c2 = (int)w2_shape[1];
  if ((size_t)r1 * (size_t)r2 != rows || (size_t)c1 * (size_t)c2 != k)
    return fail(MC_EINVAL, "LoKr '%s': [%d, %d] (x) [%d, %d] is no factorisation of [%zu, %zu]", weight_name, r1, c1, r2, c2, rows, k);
  if (other_terms(adapter, weight_name, AdapterExtra::KRON) + 1 > (size_t)kLoraMaxTerms)
    return fail(MC_EINVAL, "LoKr '%s': more than %d adapters on one weight", weight_name, kLoraMaxTerms);
  AdapterExtra x;
  x.adapter = adapter; x.target = weight_name; x.kind = AdapterExtra::KRON; x.factor = factor;
  x.r1 = r1; x.c1 = c1; x.r2 = r2; x.c2 = c2;
  const void* src[2] = {w1_dev, w2_dev};
  const size_t numel[2] = {(size_t)r1 * c1, (size_t)r2 * c2};
  return store_extra(x, *s, src, numel, 2, dtype, stream);
}

mc_status WeightStore::lora_set_hada(const char* adapter, const char* weight_name, const void* u1_dev, const int64_t* u_shape,
                                     const void* d1_dev, const int64_t* d_shape, const void* u2_dev, const void* d2_dev, mc_dtype dtype,
                                     float factor, hipStream_t stream) {
  if (!adapter || !weight_name || !u1_dev || !u_shape || !d1_dev || !d_shape || !u2_dev || !d2_dev) return fail(MC_EINVAL, "null argument");
  Slot* s = nullptr;
  MC_TRY(extra_target("LoHa", weight_name, &s));
  const size_t k = (size_t)s->lin->k_in, rows = s->numel / k;
  if (u_shape[1] < 1 || u_shape[1] > (1 << 20) || d_shape[0] != u_shape[1])
    return fail(MC_EINVAL, "LoHa '%s': [%lld, %lld] and [%lld, %lld] share no rank", weight_name, (long long)u_shape[0],
                (long long)u_shape[1], (long long)d_shape[0], (long long)d_shape[1]);
  const int rank = (int)u_shape[1];
  if (u_shape[0] != (int64_t)rows || d_shape[1] != (int64_t)k)
    return fail(MC_EINVAL, "LoHa '%s': factors for a [%lld, %lld] weight, the weight is [%zu, %zu]", weight_name, (long long)u_shape[0],
                (long long)d_shape[1], rows, k);
  if (other_terms(adapter, weight_name, AdapterExtra::HADA) + 1 > (size_t)kLoraMaxTerms)
    return fail(MC_EINVAL, "LoHa '%s': more than %d adapters on one weight", weight_name, kLoraMaxTerms);
  AdapterExtra x;
  x.adapter = adapter; x.target = weight_name; x.kind = AdapterExtra::HADA; x.factor = factor; x.rank = rank;
  const void* src[4] = {u1_dev, d1_dev, u2_dev, d2_dev};
  const size_t numel[4] = {rows * (size_t)rank, (size_t)rank * k, rows * (size_t)rank, (size_t)rank * k};
  return store_extra(x, *s, src, numel, 4, dtype, stream);
}

mc_status WeightStore::lora_set_magnitude(const char* adapter, const char* weight_name, const void* mag_dev, size_t numel, mc_dtype dtype,
                                          hipStream_t stream) {
  if (!adapter || !weight_name || !mag_dev) return fail(MC_EINVAL, "null argument");
  Slot* s = nullptr;
  MC_TRY(extra_target("DoRA", weight_name, &s));
  const size_t rows = s->numel / (size_t)s->lin->k_in;
  if (numel != rows) return fail(MC_EINVAL, "DoRA '%s': a magnitude of %zu elements, %zu output rows", weight_name, numel, rows);
  for (const AdapterExtra& o : extras)
    if (o.kind == AdapterExtra::MAGNITUDE && o.target == weight_name && o.adapter != adapter)
      return fail(MC_EINVAL, "DoRA '%s': adapter '%s' brings a magnitude, adapter '%s' already has one on this weight (one magnitude "
                             "normalises a weight)", weight_name, adapter, o.adapter.c_str());
  AdapterExtra x;
  x.adapter = adapter; x.target = weight_name; x.kind = AdapterExtra::MAGNITUDE;
  const void* src[1] = {mag_dev};
  return store_extra(x, *s, src, &numel, 1, dtype, stream);
}

mc_status WeightStore::lora_set_delta(const char* adapter, const char* param_name, const void* delta_dev, size_t numel, mc_dtype dtype,
                                      hipStream_t stream) {
  auto it = slots.find(param_name);
  if (it == slots.end()) return fail(MC_EINVAL, "LoRA: unknown weight '%s'", param_name);
  Slot& s = it->second;
  if (s.dst_dtype != MC_F32)
    return fail(MC_EINVAL, "LoRA: '%s' is a bf16 matrix and takes low-rank pairs only (a full-rank delta is a checkpoint, not an adapter)",
                param_name);
  if (!allow_f32_targets || s.perm_c || s.fixed) return fail(MC_EINVAL, "LoRA: '%s' takes no delta in this engine", param_name);
  if (dtype != MC_F32) return fail(MC_EINVAL, "LoRA '%s': a delta must be given as fp32", param_name);
  if (numel != s.numel) return fail(MC_EINVAL, "LoRA '%s': a delta of %zu elements, %zu expected", param_name, numel, s.numel);
  size_t at = deltas.size(), on_target = 0;
  for (size_t i = 0; i < deltas.size(); ++i) {
    if (deltas[i].target != param_name) continue;
    if (deltas[i].adapter == adapter) at = i;
    else ++on_target;
  }
  if (on_target + 1 > (size_t)kLoraMaxTerms)
    return fail(MC_EINVAL, "LoRA '%s': more than %d adapters on one weight", param_name, kLoraMaxTerms);
  LoraDelta d;
  d.adapter = adapter; d.target = param_name;
  MC_TRY(alloc(&d.delta, numel));
  bool new_base = false;
  if (mc_status st = make_base(s, stream, &new_base)) { release(d.delta); return st; }
  hipError_t err = hipMemcpyAsync(d.delta, delta_dev, numel * 4, hipMemcpyDeviceToDevice, stream);
  if (err != hipSuccess) {
    release(d.delta);
    if (new_base) drop_base(s);
    return fail(MC_EHIP, "LoRA '%s': %s", param_name, hipGetErrorString(err));
  }
  if (at < deltas.size()) {
    release(deltas[at].delta);
    deltas[at] = d;
  } else {
    deltas.push_back(d);
  }
  lora_scales.emplace(adapter, 1.f);
  lora_dirty.insert(param_name);
  return MC_OK;
}

mc_status WeightStore::lora_scale(const char* adapter, float scale) {
  auto it = lora_scales.find(adapter);
  if (it == lora_scales.end()) return fail(MC_EINVAL, "LoRA: unknown adapter '%s'", adapter);
  if (it->second == scale) return MC_OK;
  it->second = scale;
  for (const LoraPair& p : lora)
    if (p.adapter == adapter) lora_dirty.insert(p.target);
  for (const LoraDelta& d : deltas)
    if (d.adapter == adapter) lora_dirty.insert(d.target);
  for (const AdapterExtra& x : extras)
    if (x.adapter == adapter) lora_dirty.insert(x.target);
  return MC_OK;
}

mc_status WeightStore::lora_remove(const char* adapter) {
  if (adapter && !lora_scales.count(adapter)) return fail(MC_EINVAL, "LoRA: unknown adapter '%s'", adapter);
  std::vector<LoraPair> kept;
  for (const LoraPair& p : lora) {
    if (adapter && p.adapter != adapter) { kept.push_back(p); continue; }
    lora_dirty.insert(p.target);
    release(p.up); release(p.down_t);
  }
  lora.swap(kept);
  std::vector<LoraDelta> kept_d;
  for (const LoraDelta& d : deltas) {
    if (adapter && d.adapter != adapter) { kept_d.push_back(d); continue; }
    lora_dirty.insert(d.target);
    release(d.delta);
  }
  deltas.swap(kept_d);
  std::vector<AdapterExtra> kept_x;
  for (AdapterExtra& x : extras) {
    if (adapter && x.adapter != adapter) { kept_x.push_back(x); continue; }
    lora_dirty.insert(x.target);
    release_extra(x);
  }
  extras.swap(kept_x);
  if (adapter) lora_scales.erase(adapter);
  else lora_scales.clear();
  return MC_OK;
}

// an fp32 parameter: the pairs of a matrix first (base -> live), then the deltas (base, or that result, -> live)
mc_status WeightStore::apply_f32(const std::string& name, Slot& s, hipStream_t stream) {
  float* live = (float*)s.dst + s.off;
  if (!s.f32_base) return MC_OK;   // set before its first term and never touched: live is the value
  LoraTerm terms[kLoraMaxTerms];
  const float* dl[kLoraMaxTerms];
  float ds[kLoraMaxTerms];
  int n = 0, m = 0;
  bool any = false;
  for (const LoraPair& p : lora) {
    if (p.target != name) continue;
    any = true;
    const float mult = lora_scales.at(p.adapter) * p.factor;
    if (mult != 0.f) terms[n++] = LoraTerm{p.up, p.down_t, p.rank_pad, mult};
  }
  for (const LoraDelta& d : deltas) {
    if (d.target != name) continue;
    any = true;
    const float mult = lora_scales.at(d.adapter);
    if (mult != 0.f) { dl[m] = d.delta; ds[m] = mult; ++m; }
  }
  hipError_t err = hipSuccess;
  if (n > 0) {
    const size_t k = s.f32_k;
    err = launch_lora_merge_f32(s.f32_base, (long)k, live, (long)k, (int)(s.numel / k), (int)k, terms, n, stream);
    if (err == hipSuccess && m > 0) err = launch_param_delta(live, live, s.numel, dl, ds, m, stream);
  } else if (m > 0) {
    err = launch_param_delta(s.f32_base, live, s.numel, dl, ds, m, stream);
  } else {
    err = hipMemcpyAsync(live, s.f32_base, s.numel * 4, hipMemcpyDeviceToDevice, stream);
  }
  if (err != hipSuccess) return fail(MC_EHIP, "LoRA merge of '%s': %s", name.c_str(), hipGetErrorString(err));
  if (!any) drop_base(s);   // no adapter left: live is the base again, bit for bit
  return MC_OK;
}

mc_status WeightStore::lora_apply(hipStream_t stream, int* merged) {
  std::set<Linear*> touched;
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
    LoraTerm terms[kLoraMaxTerms];
    int n = 0;
    for (const LoraPair& p : lora) {
      const float m = lora_scales.at(p.adapter) * p.factor;
      if (p.target != name || m == 0.f) continue;
      terms[n++] = LoraTerm{p.up, p.down_t, p.rank_pad, m};
    }
    KronTerm krons[kLoraMaxTerms];
    HadaTerm hadas[kLoraMaxTerms];
    int nk = 0, nh = 0;
    const float* magnitude = nullptr;   // at most one per weight (lora_set_magnitude)
    for (const AdapterExtra& x : extras) {
      if (x.target != name) continue;
      const float scale = lora_scales.at(x.adapter), m = scale * x.factor;
      if (x.kind == AdapterExtra::MAGNITUDE) {
        if (scale != 0.f) magnitude = x.p[0];
      } else if (m != 0.f && x.kind == AdapterExtra::KRON) {
        krons[nk++] = KronTerm{x.p[0], x.p[1], x.r1, x.c1, x.r2, x.c2, m};
      } else if (m != 0.f) {
        hadas[nh++] = HadaTerm{x.p[0], x.p[1], x.p[2], x.p[3], x.rank, m};
      }
    }
    if (nk + nh > 0 || magnitude) {  // the general merge, over an fp32 image of the part that lives for this launch only
      float* scratch = nullptr;
      hipError_t err = hipMalloc((void**)&scratch, rows * k * sizeof(float));
      if (err != hipSuccess) return fail(MC_ENOMEM, "adapter merge of '%s': hipMalloc(%zu) failed: %s", name.c_str(), rows * k * sizeof(float), hipGetErrorString(err));
      err = launch_adapter_merge(l.w_base + s.off, (long)k, l.w + s.off, (long)k, (int)rows, (int)k, terms, n, krons, nk, hadas, nh,
                                 magnitude, scratch, stream);
      if (err == hipSuccess) err = hipStreamSynchronize(stream);
      (void)hipFree(scratch);
      if (err != hipSuccess) return fail(MC_EHIP, "adapter merge of '%s': %s", name.c_str(), hipGetErrorString(err));
    } else if (n == 0) {
      HIP_TRY(hipMemcpyAsync(l.w + s.off, l.w_base + s.off, s.numel * 2, hipMemcpyDeviceToDevice, stream));
    } else {
      hipError_t err = launch_lora_merge(l.w_base + s.off, (long)k, l.w + s.off, (long)k, (int)rows, (int)k, terms, n, stream);
      if (err != hipSuccess) return fail(MC_EHIP, "LoRA merge of '%s': %s", name.c_str(), hipGetErrorString(err));
    }
    MC_TRY(requantise(s, stream));
    touched.insert(&l);
    lora_dirty.erase(name);
  }
  for (Linear* l : touched) {  // no adapter left on any part: w is the base again, bit for bit
    bool live = false;
    for (const LoraPair& p : lora) live = live || slots.at(p.target).lin == l;
    for (const AdapterExtra& x : extras) live = live || slots.at(x.target).lin == l;
    if (!live) {
      release(l->w_base);  // hipFree waits for the copies above
      l->w_base = nullptr;
    }
  }
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
