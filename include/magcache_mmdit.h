/*
 * magcache_mmdit.h -- C ABI of the MM-DiT engine in libmagcache_hip.so: the FLUX.1 and HunyuanVideo transformer
 * forward (dual-stream joint-attention blocks followed by single-stream fused QKV/MLP blocks) with the MagCache
 * skip path, residual capture and calibration statistics.
 *
 * Reference boundary (monkey-patch surfaces, like the Wan one in magcache_hip.h):
 *   FLUX          FluxTransformer2DModel.forward = magcache_forward       MagCache4FLUX/magcache_flux.py:234-445
 *                 (class attributes cnt, num_steps, mag_ratios, K, magcache_thresh, retention_ratio,
 *                  accumulated_ratio/err/steps, previous_residual; :452-470)
 *   HunyuanVideo  HYVideoDiffusionTransformer.forward = magcache_forward  MagCache4HunyuanVideo/magcache_sample_video.py:29-160
 *                 (cnt, num_steps, ..., residual_cache; :300-330)
 *   Qwen-Image    QwenImageTransformer2DModel.forward = magcache_forward  MagCache4QwenImage/magcache_generate.py:173-253
 *   (and -Edit)   (cnt, num_steps, K, magcache_thresh, retention_ratio, accumulated_*[2], residual_cache[2]; :63-83),
 *                 MagCache4QwenImageEdit/magcache_generate.py (same functions, more image tokens)
 * Everything those functions do between their arguments and their return value is one mc_mmdit_forward call; the
 * decision rule stays on the host (scalar state, `<=`, the FLUX step-11 exclusion: see mc_rule_* in magcache_hip.h
 * and magcache_amd/mmdit.py).  FLUX's ControlNet arguments (:374-384, :416-423) are set ahead of the forward with
 * mc_mmdit_set_controlnet.  The transformer blocks themselves are upstream code (huggingface/diffusers
 * transformer_flux.py, Tencent/HunyuanVideo hyvideo/modules/models.py); the weight names below are the upstream
 * state_dict names.
 *
 * Conventions as in magcache_hip.h: *_dev pointers are caller-owned device memory, the engine owns its weight copies,
 * all scratch and the residual cache live in one caller-provided workspace, nothing allocates or synchronises during
 * a forward, calls are asynchronous on the given hipStream_t, status codes + mc_last_error().
 *
 * GEMM launches of a block (round 5; policy in csrc/gemm_bf16_v2.hip, switches "gemm_splitk" / "mmdit_two_streams" of
 * mc_set_option): the two streams of a double block are row ranges of the joint buffers, so their q|k|v, output projection and
 * MLP-out run as ONE row-split launch each when the range boundary sits on a 256-row tile boundary (FLUX; HunyuanVideo's does
 * not: two launches); a single block's [q|k|v ; MLP-in] is one launch with two destinations; the projections back to d at small
 * image sizes (<= 128 tiles of 256 x 256) are cut along K into slices summed by a second launch -- their scratch is the
 * workspace's "splitk0" / "splitk1" (mc_mmdit_buffer_info), sized with the plan from the geometry (absent at HunyuanVideo's).
 */
#ifndef MAGCACHE_MMDIT_H
#define MAGCACHE_MMDIT_H

#include "magcache_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mc_mmdit mc_mmdit;

typedef enum {
  MC_FAMILY_FLUX = 0,    /* token order [text ; image], RoPE on every token (ids), packed-latent tokens in and out */
  MC_FAMILY_HUNYUAN = 1, /* token order [image ; text], RoPE on image tokens, Conv3d (1,2,2) patch embedding,
                            SingleTokenRefiner on the text states, text attention mask (valid prefix) */
  MC_FAMILY_QWEN = 2     /* Qwen-Image / Qwen-Image-Edit: token order [text ; image], double-stream blocks only
                            (n_single == 0), no pooled vector and no guidance embedding (vec_dim == 0), weighted RMSNorm
                            on the text states before txt_in, a text length that varies per call (txt_valid <= txt_len),
                            two CFG residual slots (mc_mmdit_forward2), one GPU (sp_size 1) */
} mc_family;

typedef struct {
  int family;
  int dim, num_heads;       /* head_dim is 128 */
  int n_double, n_single;   /* 19 / 38 (FLUX.1-dev), 20 / 40 (HunyuanVideo), 60 / 0 (Qwen-Image) */
  int in_channels;          /* FLUX, Qwen-Image: 64 token features; HunyuanVideo: 16 latent channels */
  int out_channels;         /* FLUX: 64 token features; HunyuanVideo: 16 */
  int txt_dim, txt_len;     /* T5 4096 x 512 (FLUX), LLaVA 4096 x 256 (HunyuanVideo), Qwen2.5-VL 3584 x the longest
                               prompt of a sample (Qwen-Image: txt_len is the maximum, txt_valid the length of a call) */
  int vec_dim;              /* pooled CLIP text embedding, 768; Qwen-Image: 0 */
  int img_tokens;           /* FLUX: (H/16)*(W/16); HunyuanVideo: F * (H/2) * (W/2) of the latent grid below;
                               Qwen-Image-Edit: noisy tokens + reference-image tokens */
  int latent_f, latent_h, latent_w; /* HunyuanVideo latent [16, F, H, W]; FLUX: ignored */
  int refiner_depth;        /* HunyuanVideo txt_in blocks (2); FLUX: 0 */
  int calibration;          /* reserve the second residual slot calibration mode needs (per CFG branch: Qwen-Image) */
  int sp_rank, sp_size;     /* sequence parallel: this rank owns image tokens [rank, rank+1) * img_tokens / sp_size; the
                               text tokens are replicated.  0, 1 (or 0, 0) for one GPU */
  /* ---- fields behind the first layout: read by mc_mmdit_create_sized only; 0 = as before ---- */
  int fp8_linear;           /* 0: bf16 Linears (default).  2: the block Linears that read a LayerNorm or GELU output (q|k|v,
                               MLP-in and MLP-out of both streams of a double block, linear1 of a single block) keep an e4m3
                               copy with OCP MX block scales (one E8M0 byte per 32 inputs) and run on the MX matrix-core
                               GEMM, their activations quantised the same way.  3: the Linears that read the attention
                               output too (the output projections; a single block's linear2 over all of its K = 5 dim).
                               The embedders, the modulation, the HunyuanVideo token refiner and the head stay bf16.
                               An optional speed / quality mode, one GPU (sp_size 1), dim >= 512; an fp8
                               engine runs its blocks on one stream whatever "mmdit_two_streams" says.  1 (the Wan
                               engine's per-row scales) has no MM-DiT path: MC_EINVAL, as is any other value.
                               The process option "mx_fp4" turns the MX copies of modes 2 | 3 into MXFP4 (see mc_mmdit_mx_fp4). */
} mc_mmdit_config;

/* mc_mmdit_config only ever grows at its END, and a zero in a new field keeps the behaviour older callers had.
 * mc_mmdit_create is the entry point of the first layout: it reads the struct up to and including sp_size, whatever the
 * caller's header says behind it (so an fp8_linear set there is NOT seen).  mc_mmdit_create_sized takes cfg_bytes =
 * the caller's sizeof(mc_mmdit_config): between the first layout's size and this library's, a multiple of sizeof(int)
 * (MC_EINVAL otherwise); the fields the caller's struct does not have read as zeros. */
mc_status mc_mmdit_create(const mc_mmdit_config* cfg, mc_mmdit** out);
mc_status mc_mmdit_create_sized(const mc_mmdit_config* cfg, size_t cfg_bytes, mc_mmdit** out);
void mc_mmdit_destroy(mc_mmdit* e);
size_t mc_mmdit_workspace_bytes(const mc_mmdit* e);
/* Option "mx_fp4" (mc_set_option, 0 | 1; default 0): read ONCE by mc_mmdit_create / _create_sized, like mc_create reads it, and
 * kept by the engine whatever the option is set to afterwards.  With fp8_linear 2 | 3 the same Linears hold an MXFP4 copy (W4A4:
 * OCP e2m1 elements, two per byte, with the E8M0 block scales of the MX path) and run on the MXFP4 matrix-core GEMM; their
 * activations reach the workspace buffer "aq" as packed e2m1 rows of 5 dim / 2 bytes (column c at byte c / 2, "a_mx"
 * unchanged), written by the FP4 tail of the LayerNorm kernel and the GELU epilogue of MLP-in (option "fp8_fused_quant" 1, the
 * default) or by separate quantise passes (0): the same bits either way.  With fp8_linear 0 the option does nothing.  dim must
 * be a multiple of 256 and >= 512 (an even head count; MC_EINVAL names the Linear), sp_size 1.  mc_mmdit_config does not change.
 * MXFP4 is much coarser than MX fp8 (2e-1 .. 3e-1 relative L2 from the fp32 model on synthetic weights against
 * 5e-2 .. 7e-2); it is an opt-in speed / quality experiment, not judged on real weights, never a default.
 * mc_mmdit_mx_fp4: 1 when this engine's MX Linears are MXFP4, else 0. */
int mc_mmdit_mx_fp4(const mc_mmdit* e);
/* Option "mx_fp6" (mc_set_option, 0 | 1; default 0; magcache_hip.h): latched by mc_mmdit_create / _create_sized in the same way.
 * With fp8_linear 2 | 3 the same Linears hold an MXFP6 copy (W6A6: OCP e2m3 elements, 32 per 24 bytes, with the E8M0 block
 * scales of the MX path) and run on the MXFP6 matrix-core GEMM; their activations reach "aq" as packed e2m3 rows of
 * 5 dim * 3 / 4 bytes (column c in bits 6 (c % 32) .. + 5 of the 24 bytes at 24 (c / 32); "a_mx" unchanged), always written by
 * separate quantise passes: there is no fused FP6 producer, and "fp8_fused_quant" changes nothing in this mode.  dim a
 * multiple of 256 and >= 512 (MC_EINVAL names the Linear), sp_size 1, and "mx_fp4" and "mx_fp6" both 1 is MC_EINVAL (the
 * message names both options).  mc_mmdit_config does not change.  Not judged on real weights, never a default.
 * mc_mmdit_mx_fp6: 1 when this engine's MX Linears are MXFP6, else 0. */
int mc_mmdit_mx_fp6(const mc_mmdit* e);
mc_status mc_mmdit_set_workspace(mc_mmdit* e, void* ws_dev, size_t bytes);
mc_status mc_mmdit_buffer_info(const mc_mmdit* e, const char* name, size_t* offset, size_t* bytes);

/* Token geometry per call.  mc_mmdit_create fixes the family, the widths and the depths for good; the image tokens, the
 * HunyuanVideo latent grid and the text length it was given are only the FIRST geometry: one engine (one copy of the
 * weights) serves any resolution and prompt length, as the transformers it stands for do.
 *
 * mc_mmdit_geometry_bytes: the workspace a geometry would need, the engine unchanged -- to size ONE workspace for all
 * the geometries a caller will serve (take the maximum: the plan is not monotone in the token count, the split-K scratch
 * exists at small geometries only).
 *
 * mc_mmdit_set_geometry: between forwards only (MC_ESTATE between mc_mmdit_begin and mc_mmdit_end).  The geometry is
 * checked as mc_mmdit_create checks it (MC_EINVAL: counts not positive, HunyuanVideo img_tokens != F*(H/2)*(W/2), odd H or
 * W) and the workspace is planned again: mc_mmdit_workspace_bytes and every mc_mmdit_buffer_info offset are then those of
 * an engine created at the new geometry, and views into the old plan are void.  A bound workspace is kept when the new
 * plan fits its bytes; when it does not the call returns MC_EINVAL (the message names both byte counts) and the engine
 * stays as it was, usable at its old geometry.  With no workspace bound the call only plans.  Afterwards the engine is in
 * the state mc_mmdit_set_workspace leaves it in: residual caches of both branches and calibration statistics forgotten,
 * pad rows cleaned again by the next forward; the ControlNet lists are cleared (the samples had the old img_tokens) and
 * the RoPE table is the identity rotation as after mc_mmdit_create -- set the new geometry's with mc_mmdit_set_rope.
 * The call may allocate (a longer RoPE table) and synchronises the device: it is no part of a forward and must not be
 * stream-captured.  Sequence-parallel engines (sp_size > 1) keep their geometry: MC_EINVAL.  latent_f/h/w: HunyuanVideo,
 * ignored otherwise. */
mc_status mc_mmdit_geometry_bytes(const mc_mmdit* e, int img_tokens, int latent_f, int latent_h, int latent_w, int txt_len,
                                  size_t* bytes);
mc_status mc_mmdit_set_geometry(mc_mmdit* e, int img_tokens, int latent_f, int latent_h, int latent_w, int txt_len);

/* upstream state_dict names (diffusers FluxTransformer2DModel / hyvideo HYVideoDiffusionTransformer), fp32 or bf16 */
mc_status mc_mmdit_set_weight(mc_mmdit* e, const char* name, const void* src_dev, mc_dtype dtype,
                              const int64_t* shape, int ndim, mc_stream stream);
int mc_mmdit_weights_missing(const mc_mmdit* e, char* buf, size_t buflen);

/* RoPE table for the joint sequence, rows in the engine's token order: cos_dev / sin_dev are the upstream
 * "use_real" tables [n_rows, 128] (every frequency repeated twice; FluxPosEmbed(ids) / get_nd_rotary_pos_embed).
 * FLUX, Qwen-Image: n_rows = txt_len + img_tokens (text rows first; Qwen-Image: the table of the MAXIMUM text length,
 * text row j at QwenEmbedRope position max(h/2, w/2) + j, so a shorter call uses its first txt_valid rows);
 * HunyuanVideo: n_rows = img_tokens. */
mc_status mc_mmdit_set_rope(mc_mmdit* e, const float* cos_dev, const float* sin_dev, int n_rows, mc_stream stream);

/* LoRA adapters, merged on the device.  The reference forwards open with scale_lora_layers(self, lora_scale) and close with
 * unscale_lora_layers (MagCache4FLUX/magcache_flux.py:62-67, MagCache4QwenImage/magcache_generate.py:107-113); this engine keeps
 * its forward as it is -- the same launches on the same weight pointers -- and rebuilds the weights instead: every Linear an
 * adapter touches keeps its pristine bf16 weight once, and mc_mmdit_lora_apply rewrites the live one in place,
 *   W_eff = bf16(W + sum_j scale_j * factor_j * up_j down_j)
 * (per term an fp32 product on bf16 MFMAs, the fp32 sum in the order the pairs were set, one fp32 add of W, one rounding),
 * then requantises exactly the touched rows of an MX copy (fp8_linear).  A delta far below half a bf16 ulp of W is partly
 * rounded away, as with diffusers' fuse_lora on bf16 weights.
 *   mc_mmdit_lora_set    one pair of `adapter` on `weight_name`, an upstream name of mc_mmdit_set_weight such as
 *                        "transformer_blocks.3.attn.to_q.weight" (a part of a fused matrix is addressed by its own name):
 *                        down_dev [rank, in_features], up_dev [out_features of that name, rank], both fp32 or bf16 (`dtype`),
 *                        copied; factor = alpha / rank of the target.  MC_EINVAL, naming the weight, for a name that is no bf16
 *                        matrix of a GEMM (the fp32 head, a padded image embedder, norm weights, biases), for element counts that
 *                        do not fit, and for a ninth adapter on one weight.  The same (adapter, weight_name) again replaces the
 *                        pair.  A new adapter starts at scale 1.
 *   mc_mmdit_lora_scale  the adapter's scale; a term's multiplier is scale * factor, and a multiplier of 0 leaves the term out
 *   mc_mmdit_lora_remove the adapter's pairs, or with NULL every adapter's; a Linear no adapter touches any more gets its
 *                        pristine weight back bit for bit and gives the copy up (with the next apply)
 *   mc_mmdit_lora_apply  merges every part whose pairs, multipliers or base weight changed since the last apply (a few ms for
 *                        all of FLUX.1-dev).  mc_mmdit_set_weight on a touched Linear stores into the pristine
 *                        copy and needs an apply as well.
 *   mc_mmdit_lora_info   adapters known, Linears with a pristine copy, bytes of those copies (any pointer may be NULL)
 * All of them work between forwards only (MC_ESTATE between mc_mmdit_begin and mc_mmdit_end), may allocate or free device
 * memory and must not be stream-captured; a captured forward stays valid across them, since no pointer it reads moves.
 * While a change waits for its apply, mc_mmdit_begin / _forward / _forward2 return MC_ESTATE.  Residual caches and
 * calibration statistics are left alone (an adapter change never resets MagCache state in the reference either), and
 * adapters survive mc_mmdit_set_geometry.  Sequence parallel: weights are replicated, every rank makes the same calls. */
mc_status mc_mmdit_lora_set(mc_mmdit* e, const char* adapter, const char* weight_name, const void* down_dev,
                            const int64_t* down_shape, const void* up_dev, const int64_t* up_shape, mc_dtype dtype, float factor,
                            mc_stream stream);   /* both shapes are 2-D; rank = down_shape[0] */
/* LoKr and LoHa terms and DoRA magnitudes: the contracts of mc_lora_set_kron / _set_hada / _set_magnitude (magcache_hip.h), on
 * the same weight store.  Targets are the bf16 matrices mc_mmdit_lora_set takes; the fp32 head, a padded image embedder or a
 * shape that does not factor is MC_EINVAL naming the weight.  A weight that carries one of these is rebuilt by the arithmetic
 * of mc_op_adapter_merge (fp32 scratch of the part's size, allocated and freed by the apply), then its MX / fp8 rows are
 * requantised as after any merge; a weight with low-rank pairs only keeps the merge above bit for bit.  A magnitude is live
 * while its adapter's scale is not 0; a second adapter's magnitude on one weight is MC_EINVAL naming both adapters. */
mc_status mc_mmdit_lora_set_kron(mc_mmdit* e, const char* adapter, const char* weight_name, const void* w1_dev,
                                 const int64_t* w1_shape, const void* w2_dev, const int64_t* w2_shape, mc_dtype dtype, float factor,
                                 mc_stream stream);
mc_status mc_mmdit_lora_set_hada(mc_mmdit* e, const char* adapter, const char* weight_name, const void* u1_dev,
                                 const int64_t* u_shape, const void* d1_dev, const int64_t* d_shape, const void* u2_dev,
                                 const void* d2_dev, mc_dtype dtype, float factor, mc_stream stream);
mc_status mc_mmdit_lora_set_magnitude(mc_mmdit* e, const char* adapter, const char* weight_name, const void* magnitude_dev,
                                      size_t numel, mc_dtype dtype, mc_stream stream);
mc_status mc_mmdit_lora_scale(mc_mmdit* e, const char* adapter, float scale);
mc_status mc_mmdit_lora_remove(mc_mmdit* e, const char* adapter);
mc_status mc_mmdit_lora_apply(mc_mmdit* e, mc_stream stream);
mc_status mc_mmdit_lora_info(const mc_mmdit* e, int* adapters, int* linears, size_t* base_bytes);

/* FLUX ControlNet residuals (the reference keeps upstream's controlnet_block_samples, controlnet_single_block_samples and
 * controlnet_blocks_repeat, MagCache4FLUX/magcache_flux.py:374-384 and :416-423; the ControlNet itself is the caller's).
 * Every sample is a caller-owned device tensor [img_tokens, dim] of `dtype` (16-byte aligned; always the FULL tensor, like
 * img_dev: a sequence-parallel rank reads its own rows).  The engine keeps the two pointer lists, not the samples: they are
 * read by every following MC_MODE_FULL / MC_MODE_CALIB forward until the next call; (NULL, 0, NULL, 0, ..) clears them.
 * With n blocks and m samples, block i adds sample i / ceil(n / m) to its image rows after the block (text rows untouched);
 * blocks_repeat: double block i adds sample i % m (the single blocks keep the first rule).  m > n is refused.  A sample
 * on the last block is part of the cached residual and of the calibration statistics (the residual is x_final - x0,
 * taken after the add); MC_MODE_SKIP runs no block and adds nothing.  One extra launch per block that has a sample, none
 * otherwise.  MC_FAMILY_FLUX only. */
mc_status mc_mmdit_set_controlnet(mc_mmdit* e, const void* const* double_samples_dev, int n_double_samples,
                                  const void* const* single_samples_dev, int n_single_samples, mc_dtype dtype,
                                  int blocks_repeat);
/* the index rule alone (host arithmetic): the sample block `block` of n_blocks adds, or -1 where mc_mmdit_set_controlnet
 * refuses the pair (n_samples > n_blocks, or an index past the list).  blocks_repeat applies to double blocks only. */
int mc_mmdit_controlnet_index(int n_blocks, int n_samples, int block, int blocks_repeat);

/* FLUX IP-Adapters: joint_attention_kwargs["ip_adapter_image_embeds"] of the reference forwards, which run
 * encoder_hid_proj on it and hand ip_hidden_states to every block (MagCache4FLUX/magcache_flux.py; the block side is
 * diffusers' FluxIPAdapterJointAttnProcessor2_0 and MultiIPAdapterImageProjection).  Per double block, on the image rows:
 *   ip_out = sum_j scale_j[block] * softmax(q_n K_j^T / sqrt(128)) V_j,    hidden_states += ip_out
 * with q_n the image stream's q after norm_q and before RoPE, K_j | V_j = to_k_ip_j | to_v_ip_j of adapter j's projected
 * image embeds (bias, heads of 128, no RoPE, no mask, no output projection, no gate); the add comes after the block's MLP
 * and before its ControlNet sample.  The single blocks have no IP processor.  Up to MC_IP_MAX_ADAPTERS adapters of up to
 * MC_IP_MAX_KEYS keys (images x tokens per image) each.
 *   mc_mmdit_ip_adapter_add        registers adapter j = *index (0, 1, ..) under the names diffusers gives its weights after
 *                        load_ip_adapter, to be set with mc_mmdit_set_weight and reported by mc_mmdit_weights_missing:
 *                          encoder_hid_proj.image_projection_layers.{j}.image_embeds.{weight,bias}  [tokens * cross_dim, embed_dim]
 *                          encoder_hid_proj.image_projection_layers.{j}.norm.{weight,bias}          [cross_dim] fp32
 *                          transformer_blocks.{i}.attn.processor.to_k_ip.{j}.{weight,bias}          [dim, cross_dim]
 *                          transformer_blocks.{i}.attn.processor.to_v_ip.{j}.{weight,bias}          [dim, cross_dim]
 *                        cross_dim: 256 x (1, 2, 4, 5, 6, 8, 12, 16 or 20); embed_dim a multiple of 8.  Scales start at 1.
 *   mc_mmdit_ip_adapter_set_image  the image prompt of `adapter` in slot 0 or 1: embeds_dev [n_images, embed_dim] fp32 (16-byte
 *                        aligned) -> projection, affine LayerNorm (eps 1e-5), then K | V of EVERY double block into the slot's
 *                        cache [n_double][rows][2 dim] bf16.  Once per image prompt, never per forward; two slots so that the
 *                        positive and the negative image of a true-CFG pipeline alternate without recomputing.  n_images = 0
 *                        empties the adapter's slot.  MC_EINVAL for more than MC_IP_MAX_KEYS keys, MC_ESTATE while a weight
 *                        of the adapter is not set.  May allocate (a cache that grows) and then synchronises the device.
 *   mc_mmdit_ip_adapter_scale      n = 1 (every block) or n_double values; launch arguments of the following forwards, free
 *   mc_mmdit_ip_adapter_select     the slot the following forwards read; -1 = none (the state after _add)
 *   mc_mmdit_ip_adapter_clear      removes every adapter, its weights, names and caches; selection -1
 * All of them: MC_FAMILY_FLUX only, between forwards only (MC_ESTATE between mc_mmdit_begin and mc_mmdit_end).  A block in
 * which no adapter counts (nothing selected, no image in the slot, scale 0) gets no launch and no bit of any output
 * changes; otherwise one attention launch in front of the image range's head norm and one add per double block.  On the
 * last block of a model without single blocks the residual is taken after the add, as with a ControlNet sample.
 * MC_MODE_SKIP runs no block: the cached residual already holds the contribution.  Sequence parallel: keys are replicated,
 * every rank makes the same calls and attends its own rows; nothing is gathered.
 * mc_mmdit_set_geometry and mc_mmdit_set_workspace keep adapters, images, scales and selection: they depend on no token
 * geometry (keys come from the image prompt) and live outside the workspace -- unlike the ControlNet lists, which point at
 * caller tensors of the old [img_tokens, dim] and are cleared. */
mc_status mc_mmdit_ip_adapter_add(mc_mmdit* e, int embed_dim, int cross_dim, int tokens_per_image, int* index);
mc_status mc_mmdit_ip_adapter_set_image(mc_mmdit* e, int adapter, int slot, const float* embeds_dev, int n_images,
                                        mc_stream stream);
mc_status mc_mmdit_ip_adapter_scale(mc_mmdit* e, int adapter, const float* scales, int n);
mc_status mc_mmdit_ip_adapter_select(mc_mmdit* e, int slot);
mc_status mc_mmdit_ip_adapter_clear(mc_mmdit* e);

/* One transformer evaluation (the body of the reference's magcache_forward).
 *   img_dev    FLUX: packed latent tokens [img_tokens, in_channels]; HunyuanVideo: latent [16, F, H, W]   (fp32)
 *   timestep   the value the embedding sees: FLUX timestep*1000 (:303), HunyuanVideo t (:54); guidance likewise
 *   txt_dev    text states [txt_len, txt_dim] fp32; txt_valid = number of valid rows (HunyuanVideo text_mask.sum();
 *              FLUX attends all txt_len rows and ignores it).  Qwen-Image: [txt_valid, txt_dim] (only those rows are
 *              read), 0 < txt_valid <= txt_len: the attention visits exactly txt_valid text keys and all image keys
 *   vec_dev    pooled text embedding [vec_dim] fp32 (Qwen-Image: none, may be NULL; guidance is ignored)
 *   mode       MC_MODE_FULL / MC_MODE_SKIP / MC_MODE_CALIB with the meaning of magcache_hip.h (one residual slot)
 *   out_dev    FLUX: [img_tokens, out_channels] fp32; HunyuanVideo: [16, F, H, W] fp32 */
mc_status mc_mmdit_forward(mc_mmdit* e, const float* img_dev, double timestep, double guidance, const float* txt_dev,
                           int txt_valid, const float* vec_dev, mc_mode mode, float* out_dev, mc_stream stream);
/* The same forward on one of two CFG branches (cond = 0, uncond = 1), each with its own residual cache (and, with
 * calibration, its own previous residual): MC_MODE_SKIP adds the branch's cached residual, MC_MODE_CALIB compares with
 * the branch's previous one -- the reference's residual_cache[cnt % 2] (MagCache4QwenImage/magcache_generate.py:224-244).
 * branch 1 is MC_FAMILY_QWEN only; mc_mmdit_forward is branch 0.  Buffer "residual" (mc_mmdit_buffer_info) is the
 * cache of the branch of the last forward, "residual_b0" / "residual_b1" the cache of that branch. */
mc_status mc_mmdit_forward2(mc_mmdit* e, const float* img_dev, double timestep, double guidance, const float* txt_dev,
                            int txt_valid, const float* vec_dev, mc_mode mode, int branch, float* out_dev,
                            mc_stream stream);
/* The same forward in phases, for sequence parallelism: after every mc_mmdit_block_pre the caller all-gathers
 * "kv_gather" ([sp_size][Lr_pad][2*dim] bf16; this rank's image K|V rows were put into slot sp_rank) with its own
 * communicator (torch.distributed / RCCL), then calls mc_mmdit_block_post, which attends the local queries over all
 * image shards and then the (replicated) text keys, merging the two by their log-sum-exp.  Blocks: 0..n_double-1
 * double-stream, then the single-stream ones; skipped steps (MC_MODE_SKIP) go begin -> end.  mc_mmdit_end: see
 * mmdit_engine.cpp for where the sharded output lands; img_dev / the RoPE tables are always the FULL inputs. */
mc_status mc_mmdit_begin(mc_mmdit* e, const float* img_dev, double timestep, double guidance, const float* txt_dev,
                         int txt_valid, const float* vec_dev, mc_mode mode, mc_stream stream);
mc_status mc_mmdit_block_pre(mc_mmdit* e, int block, mc_stream stream);
/* optional: attention over this rank's own image shard + the text keys, to overlap the all-gather (then block_post
 * attends the remote shards only) */
mc_status mc_mmdit_block_attn_local(mc_mmdit* e, int block, mc_stream stream);
mc_status mc_mmdit_block_post(mc_mmdit* e, int block, mc_stream stream);
mc_status mc_mmdit_end(mc_mmdit* e, float* out_dev, mc_stream stream);
mc_status mc_mmdit_unpatchify(mc_mmdit* e, const float* tokens_dev, float* out_dev, mc_stream stream);
/* norm_ratio, norm_std, cos_dis of the last MC_MODE_CALIB forward (host sync) */
mc_status mc_mmdit_calib_stats(mc_mmdit* e, float out[3], mc_stream stream);
mc_status mc_mmdit_state_reset(mc_mmdit* e);

#ifdef __cplusplus
}
#endif
#endif
