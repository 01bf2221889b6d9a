/*
 * magcache_hip.h -- C ABI of libmagcache_hip.so, the MI355X (gfx950) engine behind the MagCache
 * denoising hot path.
 *
 * The reference (Zehong-Ma/MagCache) has no plugin API: its boundary is a monkey-patch surface,
 *   Model.__class__.forward = magcache_forward  + class attributes cnt / num_steps / K / ...
 *   (MagCache4Wan2.1/magcache_generate.py:896-928), called twice per step by the sampler loop
 *   (eval/magcache/experiments/Wan2.1_EVAL/wan_magcache.py:296-299).
 * Everything below `magcache_forward` -- embeds, the N DiT blocks, skip / residual capture, head --
 * is what this library replaces.  The Python shim `magcache_amd.magcache_forward` keeps the
 * reference's signature and attribute surface and binds these entry points with ctypes (see
 * INTEGRATION.md); no torch type crosses this boundary, only device pointers, sizes and a stream.
 *
 * Conventions: every pointer named *_dev is device memory owned by the caller; the engine owns its
 * weight copies and the RoPE table; scratch and the residual cache live in ONE caller-provided
 * workspace (mc_workspace_bytes / mc_set_workspace), so nothing is allocated during a forward and
 * a forward is graph-capture-safe.  All calls are asynchronous on the given hipStream_t.  One
 * engine per device, not thread-safe.  Functions return mc_status; mc_last_error() gives the text.
 */
#ifndef MAGCACHE_HIP_H
#define MAGCACHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mc_engine mc_engine;
typedef void* mc_stream; /* hipStream_t */

typedef enum {
  MC_OK = 0,
  MC_EINVAL = 1, /* shape / dtype / seq_len violation: mirrors the reference asserts
                    (magcache_generate.py:226-227, :242, :253) */
  MC_ENOMEM = 2,
  MC_EHIP = 3,   /* a HIP runtime call failed */
  MC_ESTATE = 4  /* call order violation (missing weights / workspace / cached residual) */
} mc_status;

typedef enum { MC_F32 = 0, MC_BF16 = 1 } mc_dtype;

/* forward modes: what magcache_forward does between the embeds and the head */
typedef enum {
  MC_MODE_FULL = 0,  /* run all blocks, residual_cache[branch] = x_out - x_in   (:297-301) */
  MC_MODE_SKIP = 1,  /* x = x_in + residual_cache[branch]                        (:294-295) */
  MC_MODE_CALIB = 2  /* as FULL, plus norm_ratio / norm_std / cos_dis vs the
                        previous residual of the same branch                     (:165-175) */
} mc_mode;

/* Wan DiT geometry (upstream wan/modules/model.py WanModel.__init__ arguments) + latent grid. */
typedef struct {
  int dim, ffn_dim, num_heads, num_layers;
  int in_dim, out_dim, freq_dim, text_dim, text_len;
  int latent_f, latent_h, latent_w; /* latent [in_dim, F, H, W]; patch size is (1,2,2) */
  float eps;
  int sp_rank, sp_size; /* sequence-parallel shard of the token axis; 0,1 for one GPU */
  int n_branches;       /* residual-cache slots: 2 for CFG models (cond/uncond), 1 otherwise */
  int calibration;      /* reserve the extra residual slot calibration mode needs */
  int clip_dim;         /* 0: t2v.  > 0: Wan2.1 I2V -- width of the CLIP image features (1280); the model then
                           has img_emb (MLPProj) and the k_img / v_img cross-attention branch over 257 image
                           tokens (upstream WanI2VCrossAttention), and in_dim counts the y channels (36) */
  int vace_layers;      /* 0: none.  > 0: Wan2.1 VACE -- number of control blocks (15 for 1.3B, 8 for 14B);           */
  int vace_stride;      /*   block i hints main layer i * vace_stride (2 / 5); upstream vace_layers                    */
  int vace_in_dim;      /*   channels of vace_context (96)                                                             */
  int fp8_linear;       /* 1: the three large Linears of every block (QKV, FFN-1, FFN-2) run on the fp8 (OCP e4m3) MFMA
                           path: weights quantised per output channel at mc_set_weight, activations per token on the
                           fly; a speed / quality option (~3 % relative error per GEMM), never the default.
                           2: the same Linears on MX block-scaled fp8 (one E8M0 scale per 32 input features of every
                           token and of every output channel, v_mfma_scale_f32_16x16x128_f8f6f4; mc_op_gemm_mxfp8).
                           3: as 2, and the three dim x dim Linears of every block as well (self-attention O,
                           cross-attention Q and O).  With 1..3 the LayerNorm + modulate kernel writes the e4m3 operand
                           of the GEMM it feeds directly, and with 2 / 3 the GELU epilogue of FFN-1 writes FFN-2's
                           (mc_set_option("fp8_fused_quant", 0) restores the separate quantise passes: same bits) */
  int no_context_cache; /* 1: do not reserve the text-context cache (the per-block cross-attention K|V of two prompts:
                           2 x layers x text_len x 2 dim bf16 = 0.19 GB at 1.3B, 0.84 GB at 14B); mc_set_context /
                           mc_use_context then fail with MC_ESTATE and every forward takes its context argument */
  int no_token_timesteps; /* 1: do not reserve the second modulation set and the per-token selector of
                           mc_set_token_timesteps (Wan2.2 TI2V); the call then fails with MC_ESTATE */
  int sp_phases;        /* 1: build the sequence-parallel buffers ("kv_local", "kv_gather", "attn_lse") and take the phase
                           path (mc_blocks_sp, mc_forward_sp_rccl) even with sp_size 1 -- a world of ONE: the collective
                           path, RCCL included, exercised on a single GPU (tests/test_rccl_gpu.py).  mc_forward refuses
                           such an engine like any sharded one. */
  int token_timestep_sets; /* 0: per-token timesteps carry at most two distinct values per forward (two modulation sets, as
                           before).  3..64: the engine's capacity C of distinct per-token timesteps per forward -- "temb",
                           "emod" and "ehead" hold C sets, the time chain runs batched over them and every consumer selects
                           from a table (mc_set_token_timesteps).  1, 2, > 64, or non-zero with no_token_timesteps:
                           MC_EINVAL */
} mc_config;

const char* mc_last_error(void);
const char* mc_version(void);
/* Process-wide tuning knobs (no reference counterpart; results are identical for every setting up to fp32 summation
 * order, bit-identical where noted).
 *   "gemm_kernel"   0 = chosen by shape (default): gemm_bf16_v2.hip -- 256x256 tile, 4 waves x (128 x 128), one wave per
 *                   SIMD, generated instruction stream, persistent over output tiles -- for every epilogue of shapes with
 *                   K >= 1024 whose tile count suits 256-tiles (bf16 / GELU / gated residual incl. the MagCache residual
 *                   capture and per-token gates as lean row-major epilogues, bf16 | GELU with two destinations, fp32 store);
 *                   the 128x128 kernel for everything else (small or odd shapes, K < 1024, the embed epilogues).
 *                   1 = the 128x128 kernel everywhere, 2 = the 8-wave 256x256 kernel (gemm_bf16_big.hip) wherever it
 *                   applies -- since round 5 only reachable this way: the independent implementation the parity tests
 *                   and A/B runs compare gemm_bf16_v2 with --, 4 = gemm_bf16_v2 wherever it applies.  All give the same bits.
 *   "gemm_splitk"   1 (default) = split-K by shape (see mc_op_set_splitk_workspace below), 0 = never, 2..16 = that many
 *                   slices wherever K divides (parity tests).
 *   "gemm_v2_max_grid"  0 (default) = gemm_bf16_v2 runs one persistent workgroup per CU; n = at most n (leaves CUs to a
 *                   kernel of another stream: tools/cfg_overlap_probe.py).  Same results.
 *   "gemm_defer"    no effect in the shipped library.  (A/B libraries whose gemm_bf16_v2 stream was generated with
 *                   tools/gen_gemm_v2.py --defer 1 apply a gated-residual epilogue inside the next output tile's main
 *                   loop -- bit-identical, measured 1.5-4 % slower, DESIGN 3.2 -- and 0 switches that off at run time.)
 *   "sp_attn_partials"  mc_blocks_sp can run the launches of a layer's self-attention chain (this rank's shard + one per
 *                   gather round) INDEPENDENTLY, alternating between the launch stream and an engine-owned side stream, each
 *                   into its own slot of "ao_part" / "lse_part", with one merge kernel joining them by their log-sum-exp in
 *                   fp32.  A rank's launch has 32 760 / (256 sp_size) x heads workgroups of one CU each -- 384 at sp 4, 192 at
 *                   sp 8: not whole waves of the chip's 256 CUs --, two launches side by side fill it: +11 % / +9 % on a
 *                   rank's attention alone (profiles/r06/attn_fill_probe.log), -4 % on the layer loop (sp_timeline.log).
 *                   1 (default) = where a launch fills less than 90 % of the CU slots of its waves, 2 = always, 0 = never (one stream,
 *                   every launch merged into the running result in place: what mc_block_attn_local / _round do).
 *   "attn_kernel"   0 = default dispatch = 5: attention_v5.hip (4 waves x 64 query rows, one wave per SIMD, generated
 *                   32x32x16 MFMA stream with the lazy softmax reference and the pipelined finish) for EVERY form of the
 *                   call -- one or several key shards, a shard left out, log-sum-exp out and the merge with an earlier
 *                   launch (the sequence-parallel forms) -- whose K / V span fits 32-bit byte offsets; attention_v3.hip
 *                   (8 waves x 32 rows) otherwise.  3 = attention_v3 everywhere.
 *   "fp8_fused_quant"  1 (default) = with mc_config.fp8_linear the LayerNorm + modulate kernel (and, MX modes, the GELU
 *                   epilogue of FFN-1) write the e4m3 operand of the next GEMM; 0 = separate quantise passes.  Same bits.
 *   "mx_fp4"        0 (default) | 1.  Read ONCE by mc_create / mc_create_sized; the engine keeps what it read (mc_engine_mx_fp4).
 *                   1 with mc_config.fp8_linear 2 | 3: the Linears that would hold an MX fp8 copy hold an MXFP4 copy instead
 *                   (e2m1 elements, the same E8M0 block scales) and run on mc_op_gemm_mxfp4's kernel, their activations
 *                   quantised to MXFP4 by separate passes (W4A4; no fused FP4 producer).  Coarser than MX fp8; its quality on
 *                   real weights has not been judged; never a default.  With fp8_linear 0 | 1 it does nothing.  A width the
 *                   kernel cannot tile (dim or ffn_dim no multiple of 256, or < 512) is MC_EINVAL at mc_create.  Wan engine only.
 *   "mx_fp6"        0 (default) | 1.  Read ONCE by mc_create / mc_create_sized and by mc_mmdit_create / _create_sized; the engine
 *                   keeps what it read (mc_engine_mx_fp6, mc_mmdit_mx_fp6).  1 with fp8_linear 2 | 3: the Linears that would
 *                   hold an MX fp8 copy hold an MXFP6 copy instead (OCP e2m3 elements -- the three mantissa bits of e4m3 --,
 *                   packed rows of 3 k / 4 bytes, the same E8M0 block scales) and run on mc_op_gemm_mxfp6's kernel, their
 *                   activations quantised to MXFP6 by separate passes whatever "fp8_fused_quant" says (W6A6; no fused FP6
 *                   producer).  Not judged on real weights; never a default.  With fp8_linear 0 | 1 it does nothing.  A
 *                   width the kernel cannot tile (an in_features that is no multiple of 256, or < 512) is MC_EINVAL at
 *                   create time, and so is a create with "mx_fp4" and "mx_fp6" both 1.
 *   "mmdit_two_streams"  the text stream of an MM-DiT double block (FLUX / HunyuanVideo) runs on a second HIP stream next
 *                   to the image stream between a fork and a join event.  OPT-IN (default 0 = off): 1 = on, -1 = by shape
 *                   (on when the text half is at least 1/16 of the image half and the engine is not sequence parallel);
 *                   2..6 = the diagnostic splits of tests/two_stream_bisect.py.  Round 2 traced a run-to-run difference
 *                   of this overlap to packed-fp32 VALU instructions of one kernel executing beside the other stream's
 *                   MFMA waves on one CU and removed them from the kernels involved (bit-identical since: 300-replay
 *                   test, 4000-forward soak; FLUX.1-dev 512x512: +11 %); round 4 showed that agent-scope acquire /
 *                   release and cache-bypassing loads do not change the fault (it is an ALU result, not visibility:
 *                   profiles/r04/NOTES.md 4).  The cause below that is not known, so a caller has to ask for the overlap.
 * Used by the parity tests and the A/B micro-benchmarks (tools/kbench.cpp loads several builds of this library side by side:
 * tools/build_v5_variants.py, build_gemm_v2_variants.py). */
mc_status mc_set_option(const char* key, int value);
/* the value a key holds now (a caller that sets an option around one call puts the previous value back) */
mc_status mc_get_option(const char* key, int* value);

/* ---- lifecycle ------------------------------------------------------------------------------ */
mc_status mc_create(const mc_config* cfg, mc_engine** out);
/* ABI rule for mc_config: it only grows at its END and a zero in a new field means "as before".  mc_create reads
 * sizeof(mc_config) of THIS header; a caller compiled against an older header (a shorter struct) must call
 * mc_create_sized(cfg, sizeof(mc_config) as IT knows it, out): the missing tail is taken as zeros.  History: 0.1 ends at
 * vace_in_dim, 0.2 adds fp8_linear, 0.3 no_context_cache and no_token_timesteps, 0.5 sp_phases (0.6 adds calls only: mc_pair_begin / mc_pair_end; 0.7 adds calls only: mc_geometry_bytes / mc_set_geometry,
 * mc_op_rope_axes / mc_op_rope_expand; 0.7.1 adds calls only: mc_lora_*, mc_op_lora_merge_f32, mc_op_param_delta; the MXFP4 and MXFP6 modes add calls only: mc_get_option,
 * mc_engine_mx_fp4 / _mx_fp6, mc_op_quantize_rows_mxfp4 / _mxfp6, mc_op_gemm_mxfp4 / _mxfp6); 0.8 adds token_timestep_sets (and the calls
 * mc_engine_token_timestep_sets, mc_op_gemm_bf16_resid_sets); the adapter kinds add calls only: mc_lora_set_kron / _set_hada /
 * _set_magnitude, mc_op_adapter_merge / _scratch; mc_version() names the library's. */
mc_status mc_create_sized(const mc_config* cfg, size_t cfg_bytes, mc_engine** out);
void mc_destroy(mc_engine* e);
/* 1: this engine's quantised Linears are MXFP4 (it was created under mc_set_option("mx_fp4", 1) with fp8_linear 2 | 3); else 0 */
int mc_engine_mx_fp4(const mc_engine* e);
/* the same for MXFP6 and the option "mx_fp6" (an engine is never both: such a create is MC_EINVAL) */
int mc_engine_mx_fp6(const mc_engine* e);
size_t mc_workspace_bytes(const mc_engine* e);
mc_status mc_set_workspace(mc_engine* e, void* ws_dev, size_t bytes);
/* The latent grid as a property of the call (0.7).  mc_config.latent_f / _h / _w is the grid an engine STARTS with;
 * mc_set_geometry changes it between forwards on the same weights (the reference's --size / --frame_num are per run).
 * mc_geometry_bytes = the workspace bytes the grid would need (the engine is not changed): a host that serves several grids
 * binds the MAXIMUM of their needs once and then switches without allocating.
 * mc_set_geometry:
 *   - T2V, I2V, VACE, TI2V and fp8 engines.  A sharded engine (sp_size > 1 or sp_phases) is refused with MC_EINVAL: its
 *     "kv_gather", the RCCL binding of the workspace base and the host's gather views are sized by the shard.
 *   - MC_ESTATE between mc_embed and mc_head of a phase forward.
 *   - a grid mc_create would refuse (odd H or W, ...) is refused in the same way; a plan that does not fit the bound
 *     workspace returns MC_EINVAL (the text names both byte counts) and leaves the engine untouched and usable at its
 *     old grid.
 *   - on success, in this order: hipDeviceSynchronize (earlier forwards may still read the old plan); the RoPE table and the
 *     buffer of its per-axis values grow if they have to -- the only allocation, before anything changes, never inside a
 *     forward --; the workspace is re-planned under its binding; the grid and the row counts are stored; the per-axis RoPE
 *     values (mc_op_rope_axes: a few tens of KB) are uploaded and one launch expands them to the per-token table
 *     (mc_op_rope_expand), the same bits as mc_op_rope_table.
 *   - afterwards everything that lived at an offset that may have moved is forgotten, as on a new engine: the residual
 *     caches and calibration statistics (MC_MODE_SKIP needs a new FULL forward), both text-context slots (mc_use_context
 *     returns MC_ESTATE until mc_set_context), the CLIP image context (mc_set_clip_fea again), the VACE context
 *     (mc_set_vace_context again), per-token timesteps (mc_set_token_timesteps again), a kept CFG front; offsets from
 *     mc_buffer_info are those of the new plan.  mc_set_workspace forgets the same things: other memory loses those bytes
 *     as surely as a re-plan does.
 *   - it synchronises, so it must not be stream-captured, and a graph captured before it is void (other offsets, other
 *     launch sizes).
 * An engine that is never switched runs the launches it ran before on the same bytes: every offset of its plan is unchanged. */
mc_status mc_geometry_bytes(const mc_engine* e, int latent_f, int latent_h, int latent_w, size_t* bytes);
mc_status mc_set_geometry(mc_engine* e, int latent_f, int latent_h, int latent_w);
/* named sub-buffer of the workspace (offset from ws_dev): "x", "x0", "kv_gather", "kv_local",
 * "head_tokens", "residual0", "residual1", "calib_sums", "calib_stats", ... */
mc_status mc_buffer_info(const mc_engine* e, const char* name, size_t* offset, size_t* bytes);

/* Weights by upstream state_dict name ("patch_embedding.weight", "blocks.3.self_attn.q.weight",
 * "head.modulation", ...).  The engine keeps its own copy (bf16 for the block Linears, fp32 for
 * norms / biases / modulation / time embedding / head), so src_dev may be freed afterwards. */
mc_status mc_set_weight(mc_engine* e, const char* name, const void* src_dev, mc_dtype dtype, const int64_t* shape,
                        int ndim, mc_stream stream);
int mc_weights_missing(const mc_engine* e, char* buf, size_t buflen); /* count; names into buf */

/* ---- LoRA adapters, merged into the weights on the device (0.7.1) -- the contracts of magcache_mmdit.h's mc_mmdit_lora_*, on
 * the same weight store, plus what Wan adapters need: fp32 targets and additive deltas.
 *   mc_lora_set        one low-rank pair of `adapter` on `weight_name`, a name of mc_set_weight: down [rank, in_features] and
 *                      up [rows of that weight, rank], fp32 or bf16, copied; factor = alpha / rank of the target.  Targets: every bf16
 *                      matrix of a block, of the text / image / VACE embedders, AND the fp32 matrices time_embedding.0/.2,
 *                      time_projection.1 and head.head.  A bf16 target is rebuilt as bf16(W + sum_j m_j up_j down_j) (one
 *                      rounding, mc_op_lora_merge); an fp32 target as W + sum_j m_j up_j down_j with the operands rounded to
 *                      bf16, fp32 accumulation and NO rounding of the sum (mc_op_lora_merge_f32).  patch_embedding.weight and
 *                      vace_patch_embedding.weight take no adapter.  The same (adapter, weight_name) again replaces the pair; at
 *                      most MC_LORA_MAX_TERMS adapters per weight; a new adapter starts at scale 1.
 *   mc_lora_set_delta  an additive delta of `adapter` on an fp32 parameter -- a bias (that of a part of a fused Linear by its
 *                      own name, "blocks.0.self_attn.q.bias"), a norm weight, "blocks.N.modulation", "head.modulation", an fp32
 *                      matrix: p = p0 + sum_j scale_j delta_j (mc_op_param_delta; on an fp32 matrix the pairs are merged first
 *                      and the deltas added to that).  `delta_dev`: `numel` fp32 elements (dtype must be MC_F32), copied.
 *                      Same replace rule and the same limit per parameter.  A delta on a bf16 matrix is MC_EINVAL: a
 *                      full-rank delta is a checkpoint, not an adapter.
 *   mc_lora_scale      the adapter's scale; a term's multiplier is scale * factor (deltas: factor 1), and 0 leaves it out
 *   mc_lora_remove     the adapter's terms, or with NULL every adapter's
 *   mc_lora_apply      rebuilds every parameter whose terms, multipliers or base changed since the last apply from its pristine
 *                      copy (kept while an adapter touches it; mc_set_weight on such a parameter stores into the copy), and
 *                      requantises exactly the touched rows of an fp8 Linear (fp8_linear 1, 2, 3).  A parameter no adapter
 *                      touches any more is its pristine value again, bit for bit, and its copy is freed.
 *   mc_lora_info       adapters known, parameters with a pristine copy, bytes of those copies (any pointer may be NULL)
 * Between forwards only: MC_ESTATE between mc_pair_begin and mc_pair_end, and between mc_embed and mc_head of a phased
 * forward.  They may allocate and are not capturable.  While a change waits for its apply, mc_forward, mc_embed,
 * mc_set_context, mc_set_clip_fea and mc_set_vace_context return MC_ESTATE.  An apply that rebuilt at least one parameter
 * invalidates everything the engine derived from weights: both text-context slots (the selected slot becomes -1), the CLIP
 * context, the VACE context and a kept pair front -- set them again before the next forward, which otherwise returns MC_ESTATE
 * naming what is missing.  The MagCache state (residual caches, calibration statistics) is left alone, and adapters survive
 * mc_set_geometry.  No pointer moves: a captured forward stays valid -- upload the contexts again outside the graph and replay.
 * An engine with no adapter runs the launches it always ran on the pointers it always read.  With sequence parallelism every
 * rank makes the same calls. */
mc_status mc_lora_set(mc_engine* e, const char* adapter, const char* weight_name, const void* down_dev, const int64_t* down_shape,
                      const void* up_dev, const int64_t* up_shape, mc_dtype dtype, float factor, mc_stream stream);
mc_status mc_lora_set_delta(mc_engine* e, const char* adapter, const char* param_name, const void* delta_dev, size_t numel,
                            mc_dtype dtype, mc_stream stream);
/* The other kinds of term (LyCORIS LoKr and LoHa) and the DoRA magnitude, on the bf16 matrices mc_lora_set takes (a part of a
 * fused matrix by its own name).  An fp32 matrix (time_embedding.0/.2, time_projection.1, head.head), a padded embedder or a
 * shape that does not factor is MC_EINVAL naming the weight.  Operands fp32 or bf16 (`dtype`), copied and widened to fp32.
 *   mc_lora_set_kron       m * kron(w1 [r1, c1], w2 [r2, c2]), r1 r2 = rows of the weight, c1 c2 = in_features:
 *                          element (r, c) = w1[r / r2, c / c2] * w2[r % r2, c % c2]
 *   mc_lora_set_hada       m * (u1 d1) (.) (u2 d2), element-wise; u1, u2 [rows, rank] (u_shape), d1, d2 [rank, in_features]
 *                          (d_shape)
 *   mc_lora_set_magnitude  the DoRA magnitude g [rows] (`numel` = rows) of `adapter` on the weight: with it the weight is
 *                          bf16(g[r] / |V[r, :]| * V[r, :]), V = W + every live term -- PEFT's merged DoRA weight
 *                          magnitude / |W + s B A|_row * (W + s B A).  It is live while its adapter's scale is not 0; with the
 *                          scale at 0 the adapter's terms and its magnitude are both left out.  The norm is recomputed by every
 *                          apply, so a DoRA adapter at scale 0.5 is NOT half way between W and the scale-1 weight.  Where other
 *                          adapters are live on the same weight their deltas sit inside the normalised direction (PEFT has no
 *                          merged form for that case).  One magnitude per weight: a second adapter's is MC_EINVAL naming both.
 *                          A row of V that is all zero stays zero.
 * The same (adapter, weight_name) and kind replaces; pairs, Kronecker and Hadamard terms together are at most
 * MC_LORA_MAX_TERMS per weight.  A weight that carries one of these is rebuilt by the arithmetic of mc_op_adapter_merge, with an
 * fp32 scratch of rows x in_features x 4 bytes that mc_lora_apply allocates and frees; a weight whose live terms are all
 * low-rank pairs, with no magnitude, keeps mc_op_lora_merge bit for bit.  mc_lora_scale / _remove / _apply / _info, the
 * MC_ESTATE rules and the invalidation after an apply treat these entries as they treat pairs. */
mc_status mc_lora_set_kron(mc_engine* e, const char* adapter, const char* weight_name, const void* w1_dev, const int64_t* w1_shape,
                           const void* w2_dev, const int64_t* w2_shape, mc_dtype dtype, float factor, mc_stream stream);
mc_status mc_lora_set_hada(mc_engine* e, const char* adapter, const char* weight_name, const void* u1_dev, const int64_t* u_shape,
                           const void* d1_dev, const int64_t* d_shape, const void* u2_dev, const void* d2_dev, mc_dtype dtype,
                           float factor, mc_stream stream);
mc_status mc_lora_set_magnitude(mc_engine* e, const char* adapter, const char* weight_name, const void* magnitude_dev, size_t numel,
                                mc_dtype dtype, mc_stream stream);
mc_status mc_lora_scale(mc_engine* e, const char* adapter, float scale);
mc_status mc_lora_remove(mc_engine* e, const char* adapter);
mc_status mc_lora_apply(mc_engine* e, mc_stream stream);
mc_status mc_lora_info(const mc_engine* e, int* adapters, int* params, size_t* base_bytes);

/* ---- one DiT evaluation = the body of magcache_forward (:229-305) ------------------------------
 * latent_dev : fp32 [in_dim, F, H, W]
 * t_dev      : fp32 scalar on device, or NULL to use t_host (no device sync either way)
 * context_dev: [ctx_len, text_dim] fp32 or bf16, ctx_len <= text_len (zero padded inside, :257-262), or NULL to use
 *             the cache slot selected by mc_set_context / mc_use_context
 * branch     : residual-cache slot, the reference's cnt % 2
 * out_dev    : fp32 [out_dim, F, H, W]                                                (:312)
 * Only for sp_size == 1; a sharded engine is driven through the phase calls below. */
mc_status mc_forward(mc_engine* e, const float* latent_dev, const float* t_dev, double t_host,
                     const void* context_dev, mc_dtype ctx_dtype, int ctx_len, int branch, mc_mode mode,
                     float* out_dev, mc_stream stream);

/* CFG pair (0.6).  A CFG sampler evaluates the model twice per step on the same latent and the same t (the reference's loop,
 * wan_magcache.py:296-299); only the text context differs, and the context first enters the model at layer 0's
 * cross-attention K|V.  Everything before that point -- the embeds of the latent and of t with every modulation vector, and
 * layer 0's LayerNorm + modulate, q|k|v Linear, q / k norm + RoPE, self-attention, O Linear with the gated residual, norm3,
 * cross-attention q Linear and its RMSNorm: the "front" -- is therefore computed twice on identical inputs.
 * mc_pair_begin(e) DECLARES: the next two mc_forward calls receive the same latent values, the same t and the same
 * conditioning other than the text context.  (The engine cannot find that out: a sampler updates its latent in place, so the
 * address of latent_dev proves nothing.)  The first of the two that runs its blocks then keeps the front -- "pair_x": it
 * works on this fp32 stream instead of "x" and copies it to "x" behind layer 0's O epilogue; "pair_cq": the normalised
 * cross-attention q rows; the embeds' own buffers stay as they are -- and the second continues from it at layer 0's
 * cross-attention with its own context.  The same kernels run on the same values in the same order: outputs, residual slots
 * and calibration statistics are the same bits as without the declaration.  mc_pair_end(e) closes the pair.
 * Falling back to two full forwards is always legal and never an error.  The second forward runs in full when: its
 * latent_dev, t_dev or t_host is not the first call's; the first forward was MC_MODE_SKIP (it ran no blocks); it is itself
 * MC_MODE_SKIP (the kept front is dropped unused); mc_set_weight, mc_set_workspace, mc_set_token_timesteps, mc_set_clip_fea,
 * mc_set_vace_context, mc_sp_set_chunks, mc_embed, mc_head or a block phase call ran in between; the pair has ended (a third forward
 * after the two is a full one, with or without mc_pair_end).  An engine that is sharded (sp_size > 1 or sp_phases), has VACE
 * layers, is I2V (clip_dim > 0) or runs an fp8 Linear mode accepts both calls and always runs in full; its "pair_x" /
 * "pair_cq" are 256-byte stubs.  A forward that continues from a kept front logs no profile pairs for the front
 * (mc_profile_read_classes: one MC_PROF_ATTN_SELF, GEMM_QKV, GEMM_O and GEMM_CROSS_Q pair, two LN_MODULATE and two
 * RMSNORM_ROPE pairs fewer, MC_PROF_EMBED only for a context passed by pointer); the first forward's copy is one
 * MC_PROF_OTHER pair.  Between the two forwards "x" holds the stream behind layer 0's O epilogue, not the first forward's
 * final stream (a phase call in between ends the pair, but reads that "x").  A host that never calls mc_pair_begin gets the
 * same launches and results as before; the one thing that changes for it is mc_workspace_bytes of a single-GPU bf16 T2V
 * engine, which grows by Lp * dim * 6 bytes for "pair_x" / "pair_cq" (302 MB at Wan2.1-1.3B 480p).  mc_set_geometry drops a
 * kept front like mc_set_workspace does. */
mc_status mc_pair_begin(mc_engine* e);
mc_status mc_pair_end(mc_engine* e);

/* Text-context cache.  The context is constant per CFG branch over a whole video, but the reference recomputes
 * text_embedding(context) (:256-262) and every block's cross-attention k / v of it (upstream WanT2VCrossAttention) in
 * every forward.  mc_set_context embeds `context_dev` once and stores norm_k(k(ctx)) | v(ctx) of every block in cache slot
 * `slot` (0 or 1: one per CFG branch) and selects it; mc_use_context selects a filled slot (-1: none); a forward /
 * mc_embed called with context_dev == NULL then reads the selected slot.  Passing a context pointer to the forward keeps
 * the uncached behaviour.  mc_set_weight invalidates both slots. */
mc_status mc_set_context(mc_engine* e, int slot, const void* context_dev, mc_dtype ctx_dtype, int ctx_len,
                         mc_stream stream);
mc_status mc_use_context(mc_engine* e, int slot);

/* Wan2.1 I2V: clip_fea (upstream `clip_fea`, magcache_generate.py:203,264-266) = [n_tokens (257), clip_dim]
 * fp32 or bf16.  Runs img_emb on it and keeps the image-token context for the following forwards. */
mc_status mc_set_clip_fea(mc_engine* e, const void* clip_dev, mc_dtype dtype, int n_tokens, mc_stream stream);

/* Wan2.1 VACE: vace_context [vace_in_dim, F, H, W] fp32 (reference magcache_vace_forward argument, :443, :544) and
 * vace_context_scale (:446, :546).  The patch embedding of the context is computed here, once per video; pass NULL to
 * change the scale only. */
mc_status mc_set_vace_context(mc_engine* e, const float* vace_dev, float context_scale, mc_stream stream);

/* Per-token timesteps.  The Wan2.2 forward takes t [B, seq_len] and builds e [B, seq_len, d] / e0 [B, seq_len, 6, d]
 * (MagCache4Wan2.2/magcache_generate.py:261-270).  The engine never materialises e0 (9.3 GB fp32 at 14B / 720p): it
 * evaluates the time MLP once per DISTINCT value and every consumer (LayerNorm modulation, both gated residual epilogues,
 * the head) selects a modulation set per token through one selector byte.
 *   default engine (token_timestep_sets = 0): at most TWO distinct values per forward -- the upstream TI2V pipeline passes
 *     t * mask: the conditioning frame's tokens carry 0, all others the step's t.  Set 0 = max(t), set 1 = min(t).
 *   capacity engine (token_timestep_sets = C, 3..64): up to C distinct values (one timestep per latent frame, several
 *     conditioning frames at their own noise levels).  One device pass finds the distinct values in DESCENDING order into
 *     "tok_vals" (C floats, padded with the last value found), the time chain runs once, batched over the C sets, and the
 *     consumers take row min(sel, C - 1) of the set tables.  Such an engine uses the table forms for every per-token forward,
 *     also when one or two values occur; a forward with scalar t (NULL here) runs the single-set path.
 * t_tokens_dev: fp32 [seq_len of the whole video] that must stay valid until the forward has run (it is read on the
 * forward's stream; nothing here synchronises with the host), or NULL to return to the scalar t of mc_forward.
 * "tok_t2" is the device-side record of what was found: [0] max, [1] min, [2] the number of tokens whose value received NO
 * modulation set -- neither max nor min on a default engine; beyond the capacity, or NaN, on a capacity engine, where they
 * are modulated with set C - 1 -- which must read 0, [3] (capacity engines) the number of sets in use.
 * Not defined for VACE engines (MC_EINVAL); MC_ESTATE with no_token_timesteps. */
mc_status mc_set_token_timesteps(mc_engine* e, const float* t_tokens_dev, mc_stream stream);
/* the capacity in force: token_timestep_sets, 2 for a default engine, 0 with no_token_timesteps (and for NULL) */
int mc_engine_token_timestep_sets(const mc_engine* e);

/* Measurement hook: hipEvent pairs on the launch stream around the launches of a forward, summed per class.
 * mc_profile_enable(e, 1): every SELF-attention launch (sequence parallel: the local-shard and the remote-shards launch of a
 * layer each) -- what bench.py's timed no-cache region carries for roofline.achieved.  (e, 2): every class below (a class
 * that is several launches -- the two RMSNorm + RoPE launches of q and k, the fp8 quantise + GEMM pair, the embeds, the
 * head -- is one pair around all of them); used by bench.py's separate "kernels_live" region.  (e, 0): off.  Up to 8192
 * pairs between reads; further launches are not logged.  mc_profile_read_classes waits for the logged pairs, returns
 * summed milliseconds and pair counts per class and clears the log; mc_profile_read is the self-attention class alone. */
typedef enum {
  MC_PROF_ATTN_SELF = 0,
  MC_PROF_ATTN_CROSS = 1,
  MC_PROF_GEMM_QKV = 2,     /* q | k | v Linear (bf16 store) */
  MC_PROF_GEMM_O = 3,       /* self-attention o Linear, x += gate * o (fp32 read-modify-write) */
  MC_PROF_GEMM_CROSS_Q = 4,
  MC_PROF_GEMM_CROSS_O = 5, /* cross-attention o Linear, x += o */
  MC_PROF_GEMM_FFN1 = 6,    /* Linear + GELU(tanh) */
  MC_PROF_GEMM_FFN2 = 7,    /* Linear, x += gate * y (+ the MagCache residual capture on the last layer) */
  MC_PROF_LN_MODULATE = 8,  /* the three LayerNorm (+ modulate) launches of a block */
  MC_PROF_RMSNORM_ROPE = 9,
  MC_PROF_EMBED = 10,       /* patch / time / text embeds of a forward */
  MC_PROF_HEAD = 11,        /* head LayerNorm (+ the skip add) + Linear + unpatchify */
  MC_PROF_OTHER = 12,       /* uncached text K|V, I2V image branch, calibration statistics */
  MC_PROF_SP_WAIT = 13,     /* sequence parallel (mc_blocks_sp): what a stream idled waiting for a K|V gather round = the
                               EXPOSED communication of a forward; 0 launches on one GPU.  With sp_attn_partials (default)
                               MC_PROF_ATTN_SELF is ONE pair per layer around the whole attention chain on the launch stream
                               (its launches overlap on two streams), and these waits lie INSIDE it: not additive */
  MC_PROF_NCLASS = 14
} mc_prof_class;
mc_status mc_profile_enable(mc_engine* e, int level);
mc_status mc_profile_read(mc_engine* e, double* attn_ms_total, int* attn_launches);
mc_status mc_profile_read_classes(mc_engine* e, double ms_total[MC_PROF_NCLASS], int launches[MC_PROF_NCLASS]);

/* ---- the same forward in phases (sequence parallel: the caller runs the K/V all-gather between
 * pre_attn and post_attn of every layer with its own communicator, e.g. torch.distributed/RCCL) */
mc_status mc_embed(mc_engine* e, const float* latent_dev, const float* t_dev, double t_host,
                   const void* context_dev, mc_dtype ctx_dtype, int ctx_len, mc_stream stream);
mc_status mc_block_pre_attn(mc_engine* e, int layer, mc_stream stream);  /* LN+mod, QKV, qk-norm, RoPE */
/* sp_size > 1: mc_block_pre_attn in two halves.  pre_kv = LayerNorm + the k|v Linear into "kv_local" [Lp][2 dim] + k norm /
 * RoPE -- everything the OTHER ranks wait for; pre_q = the q Linear + q norm / RoPE.  A caller that starts its all-gather
 * between the two hides it behind the q Linear as well. */
mc_status mc_block_pre_kv(mc_engine* e, int layer, mc_stream stream);
mc_status mc_block_pre_q(mc_engine* e, int layer, mc_stream stream);
/* The K|V all-gather of a layer, in C rounds (mc_sp_set_chunks; default 1).  Layout: "kv_local" [Lp][2 dim] bf16 = this
 * rank's rows (Lp = tokens per rank rounded up to 256); "kv_gather" [C][P][Lp / C][2 dim]: round c is ONE out-of-place
 * all-gather of rows [c Lp / C, (c + 1) Lp / C) of every rank's "kv_local" (contiguous send chunk, contiguous receive block).
 * The self-attention of a layer is a chain of launches merged by their log2-sum-exp in the kernel epilogue: this rank's own
 * shard first (mc_block_attn_local, needs no communication), then one launch per round as it lands (mc_block_attn_round) --
 * the attention over round c runs while round c + 1 is on the wire.  Rounds that hold padding rows only (mc_sp_round_info:
 * n_rounds < C) are neither gathered nor attended.  Lp / C must be a multiple of 64. */
mc_status mc_sp_set_chunks(mc_engine* e, int chunks);
mc_status mc_sp_round_info(const mc_engine* e, int round, int* n_rounds, int* chunk_rows, int* valid);
/* optional, sp_size > 1 only: self-attention over THIS rank's K/V shard ("kv_local", complete after pre_kv), to be
 * launched while the all-gather of the other shards is in flight; the following mc_block_attn_round / mc_block_post_attn of
 * the same layer then attend the other ranks' shards only and merge (log-sum-exp weights) */
mc_status mc_block_attn_local(mc_engine* e, int layer, mc_stream stream);
/* self-attention over gather round `round` (in order 0 .. n_rounds - 1), merged into the layer's result */
mc_status mc_block_attn_round(mc_engine* e, int layer, int round, mc_stream stream);
/* attends whatever rounds the caller has not (all of them for a caller that gathered everything first), then the rest of
 * the block */
mc_status mc_block_post_attn(mc_engine* e, int layer, int branch, mc_mode mode, mc_stream stream);
/* The same layer loop in ONE call (sp_size > 1).  For every layer in [layer_begin, layer_end) the engine runs pre_kv, calls
 * gather(user, layer, 2 c, stream) for every round c -- the caller STARTS round c of the all-gather on its own communicator,
 * ordered behind the work `stream` already holds --, runs pre_q and the local-shard attention beside them, then per round
 * gather(user, layer, 2 c + 1, s) -- the caller makes the stream `s` it is HANDED wait for round c, no host sync: the launch
 * stream, or the engine's side stream when the chain's launches alternate between the two (sp_attn_partials) -- and the
 * attention over that round; with overlap == 0 every wait comes right after the starts, on the launch stream, so that
 * nothing runs beside the collective; then post_attn.  A VACE control block follows its main layer in the same phases with its own gather.  With C = 1 the phase
 * argument is 0 (start) / 1 (wait).  The callback returns 0 on success; anything else aborts the loop with MC_ESTATE.  The
 * waits are logged as MC_PROF_SP_WAIT.  A C / C++ host calls ncclAllGather + hipStreamWaitEvent in the callback
 * (mc_blocks_sp_rccl below does exactly that), the Python shim torch.distributed (magcache_amd/parallel.py: the gloo / test
 * path).  Reference counterpart: the USP flags of MagCache4Wan2.1/magcache_generate.py:813-829,891 (xfuser). */
typedef int (*mc_sp_gather_fn)(void* user, int layer, int phase, mc_stream stream);
mc_status mc_blocks_sp(mc_engine* e, int layer_begin, int layer_end, int branch, mc_mode mode, int overlap,
                       mc_sp_gather_fn gather, void* user, mc_stream stream);
/* geometry a host of the sequence-parallel calls needs (NULL outputs are skipped): layers, tokens of the whole sequence,
 * tokens of this rank, row stride of "head_tokens" (fp32 elements), model width, sp_size; and the workspace address given to
 * mc_set_workspace (mc_buffer_info's offsets are relative to it) */
mc_status mc_sp_geometry(const mc_engine* e, int* num_layers, int* seq_len, int* rows_per_rank, int* head_stride, int* dim,
                         int* sp_size);
void* mc_workspace_base(const mc_engine* e);

/* ---- the collective inside the library (csrc/sp_rccl.cpp): an RCCL communicator held by the C side, bound at run time
 * (dlopen of the librccl already mapped into the process, else the system one: no link dependency, single-GPU users never
 * load it).  Bootstrap like any NCCL program: ONE rank calls mc_sp_comm_id, the MC_SP_ID_BYTES bytes reach the others by
 * whatever channel the host has (the Python shim: broadcast_object_list over its existing process group), every rank calls
 * mc_sp_comm_create (collective; on the calling thread's current device).  The communicator owns a high-priority stream on
 * which the gather rounds run beside the launch stream, and the events that order the two.
 * mc_blocks_sp_rccl = mc_blocks_sp with ncclAllGather + hipStreamWaitEvent as the callback;
 * mc_forward_sp_rccl = the whole sharded evaluation in ONE call: mc_embed, the layer loop, (MC_MODE_CALIB) the all-reduce
 * of "calib_sums" + mc_calib_finalize, mc_head, the all-gather of every rank's head tokens into tokens_full_dev
 * (fp32 [seq_len][head_stride], caller-owned) and mc_unpatchify -> out_dev [out_dim, F, H, W] on every rank. */
#define MC_SP_ID_BYTES 128
typedef struct mc_sp_comm mc_sp_comm;
int mc_sp_rccl_available(void); /* 1: librccl found and bound (mc_last_error() says why not) -- ask EVERY rank before the
                                   collective mc_sp_comm_create, which a rank without the library would never join */
mc_status mc_sp_comm_id(void* id_out);
mc_status mc_sp_comm_create(const void* id, int nranks, int rank, mc_sp_comm** out);
void mc_sp_comm_destroy(mc_sp_comm* c);
const char* mc_sp_comm_info(const mc_sp_comm* c); /* "rccl <version> from <library>; N ranks, rank r" */
mc_status mc_blocks_sp_rccl(mc_engine* e, mc_sp_comm* c, int layer_begin, int layer_end, int branch, mc_mode mode,
                            int overlap, mc_stream stream);
mc_status mc_forward_sp_rccl(mc_engine* e, mc_sp_comm* c, const float* latent_dev, const float* t_dev, double t_host,
                             const void* context_dev, mc_dtype ctx_dtype, int ctx_len, int branch, mc_mode mode,
                             int overlap, float* tokens_full_dev, float* out_dev, mc_stream stream);
/* VACE under sequence parallelism: control block i in the same two phases (K/V all-gather between them); call them
 * after mc_block_post_attn of main layer i * vace_stride, vace_block_post adds the hint to the main stream */
mc_status mc_vace_block_pre(mc_engine* e, int i, mc_stream stream);
mc_status mc_vace_block_post(mc_engine* e, int i, int branch, mc_mode mode, mc_stream stream);
mc_status mc_head(mc_engine* e, int branch, mc_mode mode, mc_stream stream); /* -> "head_tokens" */
/* tokens_dev: fp32 [n_tok, row stride = 4*out_dim rounded up to 64] for tokens tok0..tok0+n_tok-1 ->
 * out_dev [out_dim,F,H,W] */
mc_status mc_unpatchify(mc_engine* e, const float* tokens_dev, int tok0, int n_tok, float* out_dev,
                        mc_stream stream);

/* calibration: stats_dev[3] = {norm_ratio, norm_std, cos_dis} of the last MC_MODE_CALIB forward
 * of `branch`, found at "calib_stats" + 3*branch floats; mc_calib_finalize recomputes that triple
 * from "calib_sums" (4 doubles: sum rho, sum rho^2, sum 1-cos, count) after a cross-rank sum. */
mc_status mc_calib_ready(const mc_engine* e, int branch, int* has_stats);
mc_status mc_calib_finalize(mc_engine* e, int branch, mc_stream stream);
mc_status mc_state_reset(mc_engine* e); /* forget cached residuals (new video) */
/* residual_cache[branch] = src (fp32 [tokens of this rank, dim], device).  The reference keeps the cache
 * on the model CLASS, so Wan2.2's two experts (two model instances = two engines) read each other's
 * entries (MagCache4Wan2.2/magcache_generate.py:340-352 and the shared residual_cache[cnt%2] of :309-322);
 * the Python shim forwards an entry that lives in another engine through this call before a skip. */
mc_status mc_import_residual(mc_engine* e, int branch, const float* src_dev, mc_stream stream);

/* ---- host-side MagCache decision rule (reference :277-292, :306-311 and its per-model twins) --
 * Pure host arithmetic, never touches the device.  variant: see MC_RULE_*. */
typedef struct mc_rule mc_rule;
enum {
  MC_RULE_WAN21 = 0,     /* [2]-slot state, cnt >= int(n*R), '<'                                   */
  MC_RULE_HUNYUAN = 1,   /* scalar state, cnt >= int(R*n), '<='   (magcache_sample_video.py:88-102) */
  MC_RULE_FLUX = 2,      /* scalar, cnt >= int(R*n+0.5), '<=', step 11-of-28 never skipped
                            (magcache_flux.py:326-338)                                              */
  MC_RULE_WAN22_T2V = 3, /* [2]-slot, split_step gating (MagCache4Wan2.2/magcache_generate.py:294-303) */
  MC_RULE_WAN22_I2V = 4,
  MC_RULE_WAN22_TI2V = 5,
  /* model families outside BASELINE.json's configs, rule only */
  MC_RULE_FRAMEPACK = 6,     /* scalar, cnt >= int(R*n) and cnt >= 1, '<=', |1 - ratio| <= 0.06, re-init at cnt == 0 */
  MC_RULE_OMNIGEN2 = 7,      /* scalar (one rule object per cond / ref / uncond branch), cnt >= ceil(R*n), '<=',
                                accumulated_steps starts at 3 */
  MC_RULE_QWEN = 8,          /* Wan2.1 rule without the accumulator reset at wrap-around (Qwen-Image / -Edit) */
  MC_RULE_EVAL_WAN = 9,      /* [2]-slot, t >= int(n*0.2), '<=', table index t - 10 (sqrt-smoothed ratios) */
  MC_RULE_EVAL_OPENSORA = 10 /* scalar, t >= int(R*n), '<=', signed error 1 - acc, table index t - 1 */
};
mc_rule* mc_rule_create(int variant, int num_steps, double thresh, int K, double retention_ratio,
                        const double* mag_ratios, int n_ratios, int split_step);
void mc_rule_destroy(mc_rule* r);
/* One forward call: returns 1 if this call is skipped, 0 if the blocks run; *branch = state slot.
 * Advances cnt and resets at cnt >= num_steps exactly like the reference. */
int mc_rule_step(mc_rule* r, int* branch);
int mc_rule_cnt(const mc_rule* r);
void mc_rule_state(const mc_rule* r, double acc_err[2], int acc_steps[2], double acc_ratio[2]);
/* nearest_interp (reference :27-34); dst has target_length entries */
void mc_nearest_interp(const double* src, int src_len, double* dst, int target_length);

/* ---- single ops, exported for parity tests and micro-benchmarks --------------------------------
 * gemm: C[M,N] = A[M,K] . W[N,K]^T  bf16 in, fp32 accumulate; epi: 0 bf16(+bias) 1 gelu_tanh->bf16
 *       2 X += gate*bf16(acc+bias)  3 as 2 and R = X - X0  4 embed (X fp32, X0 bf16)  5 fp32 store
 *       MC_EINVAL, nothing launched and nothing written, unless: M > 0, N % 4 == 0, K % 64 == 0; A and W non-null and 16-byte
 *       aligned with lda, ldw >= K and % 8 == 0; bias and gate null or 16-byte aligned; every buffer the epilogue reads or
 *       writes non-null, its leading dimension >= N and % 4 == 0, bf16 buffers 8-byte and fp32 buffers 16-byte aligned (the
 *       same holds for the other gemm_bf16 forms below; the contract is stated once, at gemm_bf16_args_ok in csrc/ops.h) */
mc_status mc_op_gemm_bf16(const void* A_dev, long lda, const void* W_dev, long ldw, const float* bias_dev, int M,
                          int N, int K, int epi, void* Cb_dev, long ldc, float* X_dev, long ldx,
                          const float* gate_dev, const void* X0_dev, long ldx0, float* R_dev, long ldr,
                          void* X0out_dev, long ldx0out, int m_valid, mc_stream stream);
/* the gated-residual epilogues with PER-TOKEN gates (Wan2.2 TI2V: two timesteps per forward, mc_set_token_timesteps):
 * X[m] += (gate_sel[m] ? gate2 : gate) * bf16(acc + bias); capture != 0: and R = X_new - X0 (MagCache residual capture,
 * MagCache4Wan2.2/magcache_generate.py:309-322).  gate_sel: one byte per row. */
mc_status mc_op_gemm_bf16_resid_sel(const void* A_dev, long lda, const void* W_dev, long ldw, const float* bias_dev, int M,
                                    int N, int K, int capture, float* X_dev, long ldx, const float* gate_dev,
                                    const float* gate2_dev, const unsigned char* gate_sel_dev, const void* X0_dev, long ldx0,
                                    float* R_dev, long ldr, mc_stream stream);
/* ... with a TABLE of gate vectors (an engine with token_timestep_sets): X[m] += gates[min(sel[m], n_sets - 1) * gate_stride + n]
 * * bf16(acc + bias); capture != 0: and R = X_new - X0.  n_sets 1..64, gate_stride >= N and a multiple of 4 floats; the
 * selector byte is clamped before it forms an address.  MC_EINVAL, and nothing launched, otherwise. */
mc_status mc_op_gemm_bf16_resid_sets(const void* A_dev, long lda, const void* W_dev, long ldw, const float* bias_dev, int M,
                                     int N, int K, int capture, float* X_dev, long ldx, const float* gates_dev,
                                     long gate_stride, int n_sets, const unsigned char* sel_dev, const void* X0_dev, long ldx0,
                                     float* R_dev, long ldr, mc_stream stream);
/* two Linears with the same shapes over two ROW RANGES of the same buffers as one launch: rows [0, m_split) multiply with W
 * (+ bias, gate), rows [m_split, M) with W_b (+ bias_b, gate_b) -- the text and the image stream of an MM-DiT double block are
 * row ranges of the joint buffers (MagCache4FLUX/magcache_flux.py:342-387 calls them through diffusers' FluxTransformerBlock).
 * epi 0 bf16, 1 GELU, 2 gated residual.  One gemm_bf16_v2 launch when m_split is a multiple of 256, otherwise the two launches
 * it replaces -- the same bits either way (split-K shapes: the same bits as the two split launches only up to summation order). */
mc_status mc_op_gemm_bf16_rowsplit(const void* A_dev, long lda, const void* W_dev, const void* W_b_dev, long ldw,
                                   const float* bias_dev, const float* bias_b_dev, int M, int N, int K, int m_split, int epi,
                                   void* Cb_dev, long ldc, float* X_dev, long ldx, const float* gate_dev, const float* gate_b_dev,
                                   mc_stream stream);
/* two Linears over the same rows as one launch: columns [0, n_split) -> Cb = bf16(acc + bias), columns [n_split, N) ->
 * Cb2[m][n - n_split] = bf16(gelu_tanh(bf16(acc + bias))) (the single block of an MM-DiT: q|k|v and MLP-in,
 * MagCache4FLUX/magcache_flux.py:389-421 calls it through diffusers' FluxSingleTransformerBlock).  One gemm_bf16_v2 launch
 * where that kernel serves the shape, otherwise the two launches it replaces -- the same bits either way. */
mc_status mc_op_gemm_bf16_gelu_split(const void* A_dev, long lda, const void* W_dev, long ldw, const float* bias_dev, int M,
                                     int N, int K, int n_split, void* Cb_dev, long ldc, void* Cb2_dev, long ldc2,
                                     mc_stream stream);
/* which kernel mc_op_gemm_bf16 (and the engine) runs for this problem under the current "gemm_kernel" option: 1 = the 128x128
 * kernel, 2 = the 8-wave 256x256 kernel, 4 = gemm_bf16_v2; 0 = the shape is rejected.  (lda = ldw = K, ldc / ldx = N.) */
int mc_op_gemm_bf16_kernel(int M, int N, int K, int epi);
/* Split-K (gemm_bf16_v2): when a problem's 256 x 256 tiles cover at most half of the CUs and K is long (the M = 512 .. 1536
 * projections back to d of an MM-DiT block at image sizes: N = 3072, K = 12288 / 15360), the K loop is cut into S slices, S x
 * tiles workgroups park their fp32 accumulators in a scratch buffer and a second launch sums the slices in index order and
 * applies the epilogue (deterministic; not bit-identical to the unsplit summation order).  The engines carry the scratch in
 * their workspace ("splitk0" / "splitk1"); the single-op entry point uses the buffer set here (NULL: never split).
 * mc_op_gemm_bf16_splitk = the number of slices mc_op_gemm_bf16 would use for this problem now (1 = no split; contiguous
 * operands assumed); mc_op_gemm_splitk_need = scratch bytes the by-shape policy wants for it (0 = it does not split). */
mc_status mc_op_set_splitk_workspace(void* ws_dev, size_t bytes);
int mc_op_gemm_bf16_splitk(int M, int N, int K, int epi);
size_t mc_op_gemm_splitk_need(int M, int N, int K, int epi);
/* fp8 path (OCP e4m3, v_mfma_f32_32x32x64_f8f6f4): row-wise quantisation q = e4m3(x / s), s = max|row| / 448, and
 * C = (A_q W_q^T) * a_scale[m] * w_scale[n] + bias with the bf16 / gelu / residual-gate / fp32 epilogues */
mc_status mc_op_quantize_rows_fp8(const void* x_dev, mc_dtype dtype, long ldx, int M, int K, void* q_dev, long ldq,
                                  float* scale_dev, mc_stream stream);
mc_status mc_op_gemm_fp8(const void* A_q_dev, long lda, const float* a_scale_dev, const void* W_q_dev, long ldw,
                         const float* w_scale_dev, const float* bias_dev, int M, int N, int K, int epi, void* Cb_dev,
                         long ldc, float* X_dev, long ldx, const float* gate_dev, mc_stream stream);
/* MX block-scaled fp8 (OCP microscaling: e4m3 elements, one E8M0 scale byte per (row, 32 consecutive k), multiplied by the
 * matrix core: v_mfma_scale_f32_16x16x128_f8f6f4; mc_config.fp8_linear = 2).  Scales are stored block-major:
 * scales[kb * rows_pad + row].  quantize: e = ceil(log2(max|block| / 448)) (clamped to [-127, 127]), q = e4m3(x * 2^-e),
 * scale byte e + 127.  gemm: C = sum_kb 2^(sa - 127) 2^(sw - 127) (A_q[:, kb] . W_q[:, kb]^T) + bias, same epilogues. */
mc_status mc_op_quantize_rows_mx(const void* x_dev, mc_dtype dtype, long ldx, int M, int K, void* q_dev, long ldq,
                                 void* scales_dev, long rows_pad, mc_stream stream);
mc_status mc_op_gemm_mxfp8(const void* A_q_dev, long lda, const void* a_scales_dev, long rows_pad_a, const void* W_q_dev,
                           long ldw, const void* w_scales_dev, long rows_pad_w, const float* bias_dev, int M, int N, int K,
                           int epi, void* Cb_dev, long ldc, float* X_dev, long ldx, const float* gate_dev,
                           mc_stream stream);
/* MXFP4 (OCP microscaling: e2m1 elements -- magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6, bit 3 of a code the sign --, the same E8M0
 * scale image as MX fp8, both operands FP4 on v_mfma_scale_f32_16x16x128_f8f6f4; the Wan engine's option "mx_fp4").  Two codes
 * per byte, the EVEN k in the LOW nibble: a row of K elements is K / 2 bytes, and lda / ldw / ldq count BYTES of packed rows.
 * quantize: e = ceil(log2(max|block| / 6)) (clamped to [-127, 127]; an all-zero block: -127), code = e2m1(x * 2^-e) rounded to
 * nearest, a tie to the even mantissa; K % 32 == 0, ldx % 8 == 0, ldq % 16 == 0, 16-byte aligned pointers, rows_pad >= M
 * rounded up to 64.  gemm: M > 0 (any), N % 256 == 0, K a multiple of 256 ELEMENTS and >= 512, lda / ldw % 16 == 0 and
 * >= K / 2, 16-byte aligned operands, rows_pad_a >= M rounded up to 256, rows_pad_w >= N, both multiples of 64; no byte of A
 * behind row M - 1 is read, scale bytes are read up to rows_pad_a's first ceil256(M) rows, rows >= M of every output stay
 * untouched.  Epilogues MC_EPI_BF16, _GELU_BF16, _RESID_GATE, _F32 (as mc_op_gemm_mxfp8).  Anything else: MC_EINVAL, and
 * nothing is launched or written. */
mc_status mc_op_quantize_rows_mxfp4(const void* x_dev, mc_dtype dtype, long ldx, int M, int K, void* q_dev, long ldq,
                                    void* scales_dev, long rows_pad, mc_stream stream);
mc_status mc_op_gemm_mxfp4(const void* A_q_dev, long lda, const void* a_scales_dev, long rows_pad_a, const void* W_q_dev,
                           long ldw, const void* w_scales_dev, long rows_pad_w, const float* bias_dev, int M, int N, int K,
                           int epi, void* Cb_dev, long ldc, float* X_dev, long ldx, const float* gate_dev,
                           mc_stream stream);
/* MXFP6 (OCP microscaling: e2m3 elements -- sign, two exponent bits of bias 1, three mantissa bits: magnitudes 0 .. 0.875 by
 * 0.125, 1 .. 1.875 by 0.125, 2 .. 3.75 by 0.25, 4 .. 7.5 by 0.5, bit 5 of a code the sign --, the same E8M0 scale image as MX
 * fp8, both operands FP6 on v_mfma_scale_f32_16x16x128_f8f6f4; both engines' option "mx_fp6").  The 32 codes of a block are ONE
 * little-endian bit stream of 24 bytes: bit b (bit b % 8 of byte b / 8) is bit b % 6 of the code of k = b / 6, so code i starts
 * at bit 6 i and four codes fill three bytes.  A row of K elements is 3 K / 4 bytes, and lda / ldw / ldq count BYTES of packed
 * rows.  quantize: e = ceil(log2(max|block| / 7.5)) (clamped to [-127, 127]; an all-zero block: -127), code = e2m3(x * 2^-e)
 * rounded to nearest, a tie to the even mantissa, the sign bit x's own; any M > 0, K % 32 == 0, ldx % 8 == 0, ldq % 16 == 0 and
 * >= 3 K / 4, 16-byte aligned pointers, rows_pad >= M rounded up to 64.  gemm: M > 0 (any), N % 256 == 0, K a multiple of 256
 * ELEMENTS and >= 512, lda / ldw % 16 == 0 and >= 3 K / 4, 16-byte aligned operands, rows_pad_a >= M rounded up to 256,
 * rows_pad_w >= N, both multiples of 64; no byte of A behind row M - 1 is read, scale bytes are read up to rows_pad_a's first
 * ceil256(M) rows, rows >= M of every output stay untouched.  Epilogues MC_EPI_BF16, _GELU_BF16, _RESID_GATE, _F32 (as
 * mc_op_gemm_mxfp8).  Anything else: MC_EINVAL, and nothing is launched or written. */
mc_status mc_op_quantize_rows_mxfp6(const void* x_dev, mc_dtype dtype, long ldx, int M, int K, void* q_dev, long ldq,
                                    void* scales_dev, long rows_pad, mc_stream stream);
mc_status mc_op_gemm_mxfp6(const void* A_q_dev, long lda, const void* a_scales_dev, long rows_pad_a, const void* W_q_dev,
                           long ldw, const void* w_scales_dev, long rows_pad_w, const float* bias_dev, int M, int N, int K,
                           int epi, void* Cb_dev, long ldc, float* X_dev, long ldx, const float* gate_dev,
                           mc_stream stream);
/* attention: head_dim 128; Q rows Lq_pad (multiple of 256); KV = n_shards shards of shard_rows rows
 * (multiple of 64), the first shard_valid of each valid */
mc_status mc_op_attention(const void* Q_dev, long ldq, const void* K_dev, long ldk, long k_shard_stride,
                          const void* V_dev, long ldv, long v_shard_stride, void* O_dev, long ldo, int Lq_pad,
                          int n_heads, int shard_rows, int shard_valid, int n_shards, float scale,
                          mc_stream stream);
/* two-phase form (sequence parallel): skip_shard >= 0 leaves that shard out; lse_out [n_heads][Lq_pad] fp32 receives
 * the log2-sum-exp of the keys visited; lse_in != NULL merges with the result already in O_dev (see
 * mc_block_attn_local) */
mc_status mc_op_attention_partial(const void* Q_dev, long ldq, const void* K_dev, long ldk, long k_shard_stride,
                                  const void* V_dev, long ldv, long v_shard_stride, void* O_dev, long ldo,
                                  int Lq_pad, int n_heads, int shard_rows, int shard_valid, int n_shards,
                                  float scale, int skip_shard, float* lse_out_dev, const float* lse_in_dev,
                                  mc_stream stream);
/* the join of the two-stream attention chain (sequence parallel, sp_attn_partials): out[row, head] = sum_i w_i O_i / sum_i w_i
 * with w_i = 2^(lse_i[head][row] - max_i lse_i) over n (1..9) normalised partial results on disjoint key sets; o_parts / lse_parts
 * are HOST arrays of n device pointers (bf16 [rows][ldo] each / fp32 [d / 128][rows_pad] each, log2 units) */
mc_status mc_op_attn_merge(const void* const* o_parts, const float* const* lse_parts, int n, void* out_bf16_dev, long ldo,
                           int rows, int rows_pad, int d, mc_stream stream);
mc_status mc_op_ln_modulate(const float* x_dev, long ldx, const void* x0_dev, long ldx0, const float* sc_dev,
                            const float* sh_dev, int mode, float eps, void* out_bf16_dev, long ldo,
                            float* out_f32_dev, long ldof, int M, int D, mc_stream stream);
mc_status mc_op_rmsnorm_rope(void* x_bf16_dev, long ldx, const float* w_dev, float eps, const float* cs_dev,
                             int cs_row0, int M, int D, mc_stream stream);
/* out = float(x0) + r and r = x - float(x0), one fp32 operation per element.  MC_EINVAL, and nothing launched, for D % 8 != 0,
 * ldx0 % 8 != 0, an fp32 leading dimension that is no multiple of 4, an x0 that is not 8-byte aligned or an fp32 pointer that
 * is not 16-byte aligned. */
mc_status mc_op_skip_add(const void* x0_bf16_dev, long ldx0, const float* r_dev, long ldr, float* out_dev, long ldo,
                         int M, int D, mc_stream stream);
mc_status mc_op_residual_sub(const float* x_dev, long ldx, const void* x0_bf16_dev, long ldx0, float* r_dev,
                             long ldr, int M, int D, mc_stream stream);
/* x[m, :] += s[m, :] for m < rows: a ControlNet sample (fp32 or bf16, contiguous [rows, D], widened exactly) added to rows
 * of an fp32 stream, bitwise x + float(s).  r_dev != NULL is a second destination in the same pass: r += s, or, with
 * x0_bf16_dev != NULL, r = x_new - x0 (the MagCache residual taken after the add).  MC_EINVAL for D % 8 != 0 or a pointer
 * that is not 16-byte aligned. */
mc_status mc_op_add_rows(float* x_dev, long ldx, const void* s_dev, mc_dtype s_dtype, float* r_dev, long ldr,
                         const void* x0_bf16_dev, long ldx0, int rows, int D, mc_stream stream);
/* IP-Adapter cross-attention of the FLUX double block (diffusers FluxIPAdapterJointAttnProcessor2_0), one launch:
 *   out[m, head] = sum_j scale_j * softmax(q_n[m, head] K_j[head]^T / sqrt(128)) V_j[head]     m < rows, bf16 [rows, heads * 128]
 * q_bf16_dev: the RAW q rows (before the per-head norm), normalised per head of 128 by the kernel itself exactly as the
 * engine's head norm does without a RoPE table, q_n = bf16(bf16(q * rstd) * wq) with wq_dev [128] fp32; adapter j (1 to
 * MC_IP_MAX_ADAPTERS of them) is rows of [K | V] bf16 with leading dimension ld >= 2 * heads * 128, the first `valid`
 * (1..MC_IP_MAX_KEYS) being its keys -- rows behind them are never read.  Softmax per adapter in fp32, P rounded to bf16 for
 * P V on the matrix cores, the sum over the adapters in fp32, one rounding to bf16.  An adapter with scale 0 is skipped.
 * MC_EINVAL, and nothing launched, for an adapter or key count out of range, rows < 1, a pointer that is not 16-byte aligned
 * or a leading dimension that is too short or no multiple of 8. */
#define MC_IP_MAX_ADAPTERS 4
#define MC_IP_MAX_KEYS 256
typedef struct mc_ip_keys {
  const void* kv;
  long ld;
  int valid;
  float scale;
} mc_ip_keys;
mc_status mc_op_ip_attention(const void* q_bf16_dev, long ldq, const float* wq_dev, float eps, const mc_ip_keys* adapters,
                             int n_adapters, void* out_bf16_dev, long ldo, int rows, int heads, mc_stream stream);
/* One launch: per-token ratios + the cross-block reduction by the last block to arrive.  partial_dev: 4*n_blocks + 1
 * doubles of scratch whose LAST 8 bytes (the arrival ticket) must be zero before the first call -- the kernel rearms it;
 * sums_dev: 4 doubles (sum rho, sum rho^2, sum 1-cos, count); stats_dev: 3 floats or NULL.  MC_EINVAL, and nothing written,
 * for M < 2, D % 4 != 0, n_blocks < 1, ldr / ldrp shorter than D or no multiple of 4, r_dev / rp_dev not 16-byte aligned. */
mc_status mc_op_calib_stats(const float* r_dev, long ldr, const float* rp_dev, long ldrp, int M, int D,
                            double* partial_dev, int n_blocks, double* sums_dev, float* stats_dev,
                            mc_stream stream);
mc_status mc_op_cfg_euler(const float* cond_dev, const float* uncond_dev, float guide, float dt, float* x_dev,
                          float* eps_out_dev, size_t n, mc_stream stream);
/* Qwen-Image's true-CFG step (QwenImagePipeline norm-preserving combine + FlowMatchEulerDiscreteScheduler.step), one fp32
 * pass, in place on x: per token row m < n_rows of C (<= 256) channels, comb = u + guide (c - u), v = comb * |c| / |comb|
 * (norms over the channels of the row), x[m] += dt * v with dt = sigma_next - sigma.  A row whose |comb| is 0 gets v = 0
 * (upstream: 0 / 0 = NaN).  cond / uncond rows have stride ld_pred and may hold more rows than are updated (Qwen-Image-
 * Edit: the reference-image tokens after the first n_rows). */
mc_status mc_op_cfg_norm_euler(const float* cond_dev, const float* uncond_dev, long ld_pred, float guide, float dt,
                               float* x_dev, long ldx, int n_rows, int C, mc_stream stream);
/* weighted row RMSNorm to bf16 (Qwen-Image txt_norm, eps 1e-6): out[m] = bf16(x[m] * rsqrt(mean(x[m]^2) + eps) * w) for
 * m < rows_valid; rows [rows_valid, rows) are written as zeros.  D, ldx, ldo multiples of 4. */
mc_status mc_op_rmsnorm_rows_bf16(const float* x_dev, long ldx, const float* w_dev, float eps, void* out_bf16_dev, long ldo,
                                  int rows_valid, int rows, int D, mc_stream stream);
/* out[i] = sum_j coef[j] * xs[j][i]: xs = HOST array of k (1..6) device pointers, coef = host array of k
 * floats; out may alias an operand.  The sampler's solver updates around the model call -- CFG combine and
 * the UniPC / DPM++ / Euler flow steps of the upstream pipeline (wan_magcache.py:296-310) -- are one launch
 * each. */
mc_status mc_op_lincomb(const float* const* xs_dev, const float* coef, int k, float* out_dev, size_t n,
                        mc_stream stream);
mc_status mc_op_cast_bf16(const float* src_dev, void* dst_bf16_dev, size_t n, mc_stream stream);
/* rope table the engine builds for a latent grid: fp32 [n_tok][64][2] (cos, sin), upstream
 * wan/modules/model.py rope_params + rope_apply split (d-4*(d//6), 2*(d//6), 2*(d//6)), d = 128 */
mc_status mc_op_rope_table(int F, int Hp, int Wp, int tok0, int n_tok, float* cs_host);
/* The same table in two steps, the way the engine builds its own: entry (token, i) depends on ONE of the token's grid
 * coordinates, so the host computes only the per-axis (cos, sin) pairs -- F x 22 of the frame axis, then Hp x 21 of the height
 * axis, then Wp x 21 of the width axis, each by the double expression of mc_op_rope_table -- and a kernel copies them into
 * the per-token table.  mc_op_rope_axes is host arithmetic: *n_floats = 2 (22 F + 21 Hp + 21 Wp); axes_host == NULL only
 * returns the count.  mc_op_rope_expand: axes_dev = those floats on the device; row r < n_tok of cs_dev [n_rows][64][2] is
 * global token tok0 + r, rows >= n_tok and tokens >= F Hp Wp get the identity (1, 0).  MC_EINVAL for a null pointer, a
 * non-positive size, tok0 < 0, n_tok > n_rows or a cs_dev that is not 16-byte aligned. */
mc_status mc_op_rope_axes(int F, int Hp, int Wp, float* axes_host, size_t* n_floats);
mc_status mc_op_rope_expand(const float* axes_dev, int F, int Hp, int Wp, int tok0, int n_tok, int n_rows, float* cs_dev,
                            mc_stream stream);

/* The LoRA merge the MM-DiT engine rebuilds its weights with (magcache_mmdit.h: mc_mmdit_lora_apply), on the caller's
 * buffers: out[rows, K] = bf16(base + sum_j scale_j * (up_j down_j)), base / out bf16 with row pitches ld_base / ld_out (elements),
 * term j = bf16 down [rank, K] and up [rows, rank], contiguous, any rank >= 1.  Per term an fp32 product accumulated from zero
 * on bf16 MFMAs, the fp32 delta summed in term order, ONE fp32 add of the widened base element last, one round-to-nearest-even.
 * out may alias base; nothing outside [rows, K] is written.  The call first copies both matrices into scratch in the order its
 * MFMAs read them (rank zero-padded to a multiple of 16, rows to a multiple of 32): `scratch_dev` (256-byte aligned, at least mc_op_lora_merge_scratch bytes), or with NULL an
 * allocation of its own, which makes the call synchronous.  Not a forward-path call.  MC_EINVAL, and nothing launched, for a
 * rank < 1, more than MC_LORA_MAX_TERMS terms, K or a pitch that is no multiple of 8, a base / out pointer that is not 16-byte
 * aligned, or a scratch that is too small. */
#define MC_LORA_MAX_TERMS 8
typedef struct mc_lora_term {
  const void* down;
  const void* up;
  int rank;
  float scale;
} mc_lora_term;
size_t mc_op_lora_merge_scratch(int rows, int K, const mc_lora_term* terms, int n_terms);
mc_status mc_op_lora_merge(const void* base_dev, long ld_base, void* out_dev, long ld_out, int rows, int K,
                           const mc_lora_term* terms, int n_terms, void* scratch_dev, size_t scratch_bytes, mc_stream stream);
/* The same merge into an fp32 matrix (0.7.1; what mc_lora_apply rebuilds the Wan engine's fp32 matrices with): base / out
 * fp32, the terms bf16 as above, out = base + delta with the ONE fp32 add last and no rounding step.  K and the pitches are
 * multiples of 4 here; every other rule and refusal is mc_op_lora_merge's. */
mc_status mc_op_lora_merge_f32(const float* base_dev, long ld_base, float* out_dev, long ld_out, int rows, int K,
                               const mc_lora_term* terms, int n_terms, void* scratch_dev, size_t scratch_bytes, mc_stream stream);
/* The merge of every kind of term (what mc_lora_apply / mc_mmdit_lora_apply rebuild a bf16 weight with that carries a Kronecker
 * or Hadamard term or a DoRA magnitude), on the caller's buffers.  base / out bf16 as in mc_op_lora_merge.  fp32 throughout:
 *   delta  = sum of the PAIR terms as mc_op_lora_merge_f32 forms it on a zero base (bf16 operands, fp32 MFMA accumulation)
 *   delta += scale * (w1[r / r2, c / c2] * w2[r % r2, c % c2])      KRON: one multiply for the product, one for the scale, one add
 *   delta += scale * ((u1 d1)[r, c] * (u2 d2)[r, c])                 HADA: two rank-long fp32 dot products in k order
 *   V      = fp32(base) + delta                                      ONE add of the base element, last
 *   out    = bf16(V)                                                 magnitude == NULL
 *   out    = bf16(g[r] / sqrt(sum_k V[r, k]^2) * V[r, k])            magnitude g [rows], fp32 on the device
 * Kinds are summed in this order, the terms of a kind in array order; nothing is contracted into an fma; the row's sum of
 * squares is formed in a fixed order (no atomics), so two calls give the same bits.  out may alias base; nothing outside
 * [rows, K] of out is written.  `scratch_dev`: 256-byte aligned, at least mc_op_adapter_merge_scratch bytes (rows x K x 4 for V,
 * plus the packed copies of the pairs), or NULL for an allocation of the call's own, which makes it synchronous.  Not a
 * forward-path call.  MC_EINVAL, and nothing launched, for an unknown kind, r1 * r2 != rows or c1 * c2 != K, a rank < 1, more
 * than MC_LORA_MAX_TERMS terms, the alignment and pitch rules of mc_op_lora_merge, or a scratch that is too small. */
#define MC_ADAPTER_PAIR 0
#define MC_ADAPTER_KRON 1
#define MC_ADAPTER_HADA 2
typedef struct mc_adapter_term {
  int kind;    /* MC_ADAPTER_PAIR | MC_ADAPTER_KRON | MC_ADAPTER_HADA */
  float scale;
  const void *a, *b, *c, *d; /* PAIR: a = down [rank, K], b = up [rows, rank] (bf16, as mc_lora_term); KRON: a = w1 [r1, c1],
                                b = w2 [r2, c2] (fp32); HADA: a = u1 [rows, rank], b = d1 [rank, K], c = u2, d = d2 (fp32) */
  int rank, r1, c1, r2, c2;
} mc_adapter_term;
size_t mc_op_adapter_merge_scratch(int rows, int K, const mc_adapter_term* terms, int n_terms);
mc_status mc_op_adapter_merge(const void* base_dev, long ld_base, void* out_dev, long ld_out, int rows, int K,
                              const mc_adapter_term* terms, int n_terms, const float* magnitude_dev, void* scratch_dev,
                              size_t scratch_bytes, mc_stream stream);
/* The additive rule of a parameter that is no matrix product (0.7.1): out[i] = base[i] + sum_j scales[j] * deltas[j][i], all
 * fp32, i < n, any n > 0, 1 to MC_LORA_MAX_TERMS terms (`deltas`: a HOST array of device pointers, `scales`: a host array).
 * The sum is formed from zero in term order, a multiply and an add per term, never contracted; the base element is added last.
 * A term with scale 0 is left out, and with no live term out is a copy of base.  out may alias base.  MC_EINVAL, and nothing
 * launched, for n == 0, a term count out of range, a null pointer or one that is not 4-byte aligned. */
mc_status mc_op_param_delta(const float* base_dev, float* out_dev, size_t n, const float* const* deltas, const float* scales,
                            int n_terms, mc_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGCACHE_HIP_H */
