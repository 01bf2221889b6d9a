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

mc_status WeightStore::add_f32(float*& p, const std::string& name, size_t numel) {
  MC_TRY(alloc(&p, numel));
  add(name, p, MC_F32, numel);
  return MC_OK;
}

mc_status WeightStore::alloc_linear(Linear& l, size_t n_out, size_t k_in, Quant quant) {
  l.n_out = (int)n_out; l.k_in = (int)k_in;
  MC_TRY(alloc(&l.w, n_out * k_in));
  MC_TRY(alloc(&l.b, n_out));
  if (quant != QUANT_NONE) MC_TRY(alloc(&l.q, n_out * k_in));
  if (quant == QUANT_ROW) MC_TRY(alloc(&l.q_scale, n_out));
  if (quant == QUANT_MX) MC_TRY(alloc(&l.mx, (k_in / 32) * n_out));
  return MC_OK;
}

Slot& WeightStore::add_parts(const Linear& l, const std::string& prefix, const std::vector<Part>& parts, size_t row0) {
  const size_t k = l.k_in;
  Slot* last = nullptr;
  for (const Part& part : parts) {
    add(prefix + part.name + ".bias", l.b, MC_F32, part.rows, row0);
    last = &add(prefix + part.name + ".weight", l.w, MC_BF16, part.rows * k, row0 * k);
    last->q8 = l.q; last->q8_scale = l.q_scale; last->q8_k = k; last->mx = l.mx; last->mx_rows = l.n_out;
    row0 += part.rows;
  }
  return *last;
}

mc_status WeightStore::add_linear(Linear& l, const std::string& prefix, const std::vector<Part>& parts, size_t k_in, Quant quant) {
  size_t n_out = 0;
  for (const Part& part : parts) n_out += part.rows;
  MC_TRY(alloc_linear(l, n_out, k_in, quant));
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
    float* dst = (float*)s.dst + s.off;
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
    bf16_t* dst = (bf16_t*)s.dst + s.off;
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
    if (s.q8) {  // e4m3 copy of the rows just stored
      const size_t rows = numel / s.q8_k, row0 = s.off / s.q8_k;
      if (s.mx) {  // MX: the e4m3 bytes are relative to the block scales, not to a row scale
        HIP_TRY(launch_quantize_rows_mx(dst, nullptr, (long)s.q8_k, (int)rows, (int)s.q8_k, s.q8 + s.off, (long)s.q8_k,
                                        s.mx + row0, (long)s.mx_rows, stream));
      } else {
        HIP_TRY(launch_quantize_rows_fp8(dst, nullptr, (long)s.q8_k, (int)rows, (int)s.q8_k, s.q8 + s.off, (long)s.q8_k,
                                         s.q8_scale + row0, stream));
      }
    }
  }
  s.loaded = true;
  return MC_OK;
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
