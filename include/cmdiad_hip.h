/*
 * cmdiad_hip.h -- C ABI of libcmdiad_hip.so: the MI355X (gfx950) kernels behind CMDIAD's hot path.
 *
 * Conventions (all entry points):
 *   - plain C: device pointers + sizes + a stream handle (hipStream_t passed as void*); no torch types.
 *   - the caller owns every buffer (inputs, outputs, workspace); the library never allocates,
 *     frees, retains a pointer past the call, or synchronises the device: all work is enqueued on
 *     `stream` and is stream-ordered.  Workspace sizes come from the *_workspace_bytes() queries.
 *   - return value: CMDIAD_OK (0) or a negative cmdiad_status; cmdiad_last_error() returns the
 *     message of the calling thread's last failure.  Nothing throws across the ABI.
 *   - one host thread per device, re-entrant across streams.
 *   - bf16 tensors are passed as uint16_t* (raw bfloat16 bits), row-major unless stated.
 *
 * Each function cites the reference interface (evenrose/CMDIAD file:line) it replaces.
 */
#ifndef CMDIAD_HIP_H
#define CMDIAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cmdiad_stream_t; /* hipStream_t */

typedef enum {
    CMDIAD_OK = 0,
    CMDIAD_ERR_ARG = -1,       /* null pointer / bad size / unsupported shape */
    CMDIAD_ERR_WORKSPACE = -2, /* workspace missing or too small */
    CMDIAD_ERR_LAUNCH = -3     /* HIP reported a launch error */
} cmdiad_status;

const char* cmdiad_last_error(void);
int cmdiad_abi_version(void); /* 2: cmdiad_reweight_scan's limits and workspace changed (see there); cmdiad_gemm_args gained m_count
                                 3: LayerNorm fold -- cmdiad_gemm_args gained row_scale / ln_xb / ln_part / add2, cmdiad_gemm_qkv gained
                                    row_scale, cmdiad_block_weights the folded weights, cmdiad_transformer_block_fwd its flags;
                                    cmdiad_ln_stats_finalize is new
                                 4: cmdiad_l2_min_keys_segments, cmdiad_gemm_streamk_*, cmdiad_coreset_greedy_f32, cmdiad_coreset_prepare / _round / _decode, cmdiad_im2col3x3_bf16 are new
                                 5: cmdiad_reweight_scan_pair is new; the value bits of cmdiad_l2_min_keys' keys are the squared distance with
                                    its four low mantissa bits cleared (see there)
                                 6: cmdiad_l2_min_keys / _counted / _segments gained keys2 (the runner-up per query, NULL = off);
                                    cmdiad_l2_rescore2 and cmdiad_l2_choose are new; cmdiad_normalize_cast turns a non-finite row into a
                                    row that cannot win */
/* 1 when the library is the test-only build that also contains the superseded kernel formulations (A/B references). */
int cmdiad_has_ab_variants(void);

/* ---------------------------------------------------------------------------------------------
 * Point-cloud front end
 * ------------------------------------------------------------------------------------------- */

/* Farthest point sampling + centre gather.
 * Replaces pointnet2_ops.furthest_point_sample(xyz[B,N,3] f32, npoint) -> int32[B,npoint] and
 * pointnet2_ops.gather_operation as called at models/models.py:76-77 (fps()).
 * xyz [B,N,3] f32; n_valid [B] int32 device array or NULL (= N points in every cloud; points at
 * index >= n_valid[b] are padding); idx_out [B,G] int32; center_out [B,G,3] f32 or NULL.
 * Bit-exact with oracle/cmdiad_oracle.c:orc_fps. */
size_t cmdiad_fps_workspace_bytes(int B, int N);
int cmdiad_fps(const float* xyz, const int32_t* n_valid, int B, int N, int G, int32_t* idx_out,
               float* center_out, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* k-nearest-neighbour grouping: K nearest cloud points of every centre, ascending (d2, index),
 * plus the gathered, centre-subtracted neighbourhood.
 * Replaces knn_cuda.KNN(k, transpose_mode=True)(ref[B,N,3], query[B,G,3]) -> idx int64[B,G,k]
 * (models/models.py:86,100) and the gather/subtract at models/models.py:105-112.
 * idx_out [B,G,K] int64 (NULL allowed), neigh_out [B,G,K,3] f32 (NULL allowed).  K <= 128 and K <= N
 * (every cloud, i.e. K <= n_valid[b], must hold at least K points: the reference library has no defined result otherwise).
 * Bit-exact with oracle/cmdiad_oracle.c:orc_knn_group. */
int cmdiad_knn_group(const float* xyz, const int32_t* n_valid, const float* center, int B, int N, int G,
                     int K, int64_t* idx_out, float* neigh_out, cmdiad_stream_t stream);
/* The same result (bit for bit) by a NEIGHBOURHOOD search (ABI 6): the cloud is binned into a 64 x 64 grid on its two axes of
 * largest extent (counting sort, one workgroup per cloud), a wave scans the rings of cells around its centre and stops when the
 * K-th best distance is certified (no point outside the scanned square can be nearer) -- ~500 distance evaluations per centre
 * instead of N.  workspace: cmdiad_knn_workspace_bytes(B, N), 16-byte aligned.  Clouds of fewer than 2 048 points (and
 * CMDIAD_KNN_GRID=0) go through cmdiad_knn_group's streaming kernel. */
size_t cmdiad_knn_workspace_bytes(int B, int N);
int cmdiad_knn_group_ws(const float* xyz, const int32_t* n_valid, const float* center, int B, int N, int G, int K,
                        int64_t* idx_out, float* neigh_out, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* 3-nearest-centre search + inverse-distance weights for every cloud point.
 * Replaces the selection half of models/pointnet2_utils.py:45-75 (interpolating_points):
 * d = -2*a.b + |a|^2 + |b|^2 (:19-22), three smallest (:66-67), w = 1/(d+1e-8) normalised (:69-71).
 * xyz [B,N,3], center [B,S,3] -> idx3 [B,N,3] int32, w3 [B,N,3] f32.  S <= 4096. */
int cmdiad_interp3nn(const float* xyz, const int32_t* n_valid, const float* center, int B, int N, int S,
                     int32_t* idx3, float* w3, cmdiad_stream_t stream);
/* The same idx3 / w3 (bit for bit) by a NEIGHBOURHOOD search (ABI 6): the centres are binned into a 16 x 16 grid on their two axes
 * of largest extent, a point scans the rings of cells around it until its third best formula value is certified against
 * everything unscanned (with a bound on the formula's rounding) -- ~40 evaluations per point instead of S.
 * workspace: cmdiad_interp3nn_workspace_bytes(B, S), 16-byte aligned.  S < 64 (and CMDIAD_INTERP_GRID=0) use cmdiad_interp3nn. */
size_t cmdiad_interp3nn_workspace_bytes(int B, int S);
int cmdiad_interp3nn_ws(const float* xyz, const int32_t* n_valid, const float* center, int B, int N, int S, int32_t* idx3, float* w3,
                        void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* Organised -> unorganised point cloud without zeros (feature_extractors/multiple_features.py:10-25):
 * keeps, in raster order, the pixels whose x, y and z are all non-zero.
 * organized_pc [B,3,HW] f32 -> xyz [B,Nmax,3] f32 (first n_valid[b] rows valid), nz [B,Nmax] int32 pixel
 * indices (NULL allowed), pix2pt [B,HW] int32 = point index of a pixel or -1 (NULL allowed),
 * n_valid [B] int32 (NULL allowed; counts are clamped to Nmax). */
int cmdiad_unorganize(const float* organized_pc, int B, int HW, int Nmax, float* xyz, int32_t* nz,
                      int32_t* pix2pt, int32_t* n_valid, cmdiad_stream_t stream);

/* Weighted gather half of interpolating_points (pointnet2_utils.py:72):
 *   out[b][n][:] = (F[i0]*w0 + F[i1]*w1) + F[i2]*w2,  feat [B,S,D] f32 (centre-major), out [B,N,D] f32.
 * Only needed to materialise the reference's [1,D,N] `interpolated_feature_maps` for external callers;
 * the product path uses cmdiad_xyz_patch_fused and never builds it. */
int cmdiad_interp_gather(const float* feat, const int32_t* idx3, const float* w3, const int32_t* n_valid,
                         int B, int N, int S, int D, float* out, cmdiad_stream_t stream);

/* get_xyz_patch (feature_extractors/features.py:169-184) fused with the gather above: scatter into the
 * size x size map at nonzero pixels, AvgPool2d(3, stride 1), AdaptiveAvgPool2d((P,P)), reshape to
 * [P*P, D]; optionally the scalar normalisation (x - mean) * inv_std of multiple_features.py:976 and a
 * bf16 copy for the distance GEMM.  pix2pt [B, size*size] from cmdiad_unorganize.
 * patch_f32 [B,P*P,D] (NULL allowed), patch_bf16 [B,P*P,D] (NULL allowed). */
int cmdiad_xyz_patch_fused(const float* feat, const int32_t* idx3, const float* w3, const int32_t* pix2pt,
                           int B, int N, int S, int D, int size, int P, float mean, float inv_std,
                           float* patch_f32, uint16_t* patch_bf16, cmdiad_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Transformer / MLP building blocks (ViT-B/8: timm VisionTransformer reached at
 * models/models.py:41-52; Point-MAE: models/models.py:116-243; hallucination MLP:
 * utils/utils.py:86-115)
 * ------------------------------------------------------------------------------------------- */

/* out[M,N] = epilogue(A[M,K] . W[N,K]^T): bf16 MFMA, fp32 accumulate.  K % 64 == 0.
 * Epilogue, in order: + bias[N]; + group_bias[m / group_rows][N]; activation; + residual[M,N] (f32);
 * stores to out_f32 and/or out_bf16 (either may be NULL; out_f32 may alias residual). */
enum { CMDIAD_ACT_NONE = 0, CMDIAD_ACT_GELU = 1, CMDIAD_ACT_RELU = 2,
       CMDIAD_ACT_RELU_POST = 3 /* ReLU AFTER the residual; cmdiad_conv2d_nhwc_bf16 only */ };
typedef struct {
    const uint16_t* A; int lda;      /* [M,K] bf16 */
    const uint16_t* W; int ldw;      /* [N,K] bf16 (nn.Linear weight layout) */
    int M, N, K;
    const float* bias;               /* [N] or NULL */
    const float* group_bias;         /* [ceil(M/group_rows), N] or NULL */
    int group_rows;
    int act;
    const float* residual; int ldr;  /* [M,N] f32 or NULL */
    float* out_f32; int ldo32;
    uint16_t* out_bf16; int ldo16;
    uint16_t* out_pre_bf16;          /* [M,N] bf16 copy BEFORE the activation (training keeps z), or NULL */
    const uint16_t* dact_of;         /* [M,N] bf16 z: acc *= GELU'(z) before everything else, or NULL */
    int split_k;                     /* > 1: K is split; slab s of out_f32 ([split_k][M][ldo32]) gets partial s */
    const int* m_count;              /* ABI 2: device-resident live row count or NULL: only rows < min(M, *m_count) are computed
                                        and stored (the compacted row set of cmdiad_rows_dedup_plan: the launch is sized for M) */
    /* ABI 3, LayerNorm folded into the products on either side of it (models/models.py:177-180; all NULL = off):
     * consumer: out = act(row_scale[m] * acc + bias): W holds gamma o W centred over k, bias = b + W beta, A the RAW rows as
     * bf16 (ln_xb of the producer), row_scale = 1 / sigma per row from cmdiad_ln_stats_finalize; it must be readable up to
     * M rounded up to 256 rows (the values past M are never used). */
    const float* row_scale;
    /* producer, only with the in-place residual form (bias + residual -> out_f32, no activation, N % 64 == 0):
     * out_f32 = acc + bias + residual (+ add2); ln_xb [M, ld_xb] = the same rows as bf16; ln_part [N/64][M][2] f32 = (sum,
     * squared deviation from the chunk mean) of every 64-column chunk of every row. */
    uint16_t* ln_xb; int ld_xb;
    float* ln_part;
    const float* add2; int ld_add2;  /* second f32 addend [M,N] (the next block's positional embedding, models.py:240), or NULL */
} cmdiad_gemm_args;
int cmdiad_gemm_bf16(const cmdiad_gemm_args* args, cmdiad_stream_t stream);

/* Stream-K form of the in-place residual products of a transformer block (x = x + fc2(...), models/models.py:126-132,177-180):
 * out_f32 = A . W^T + bias + residual with N % 256 == 0, for shapes whose 256 x 256 tile count is between one and two per CU
 * (ViT-B/8's N = 768 products at batch 32: 297 tiles on 256 CUs).  The (tile, k-tile) list is cut into one contiguous range per
 * CU; a tile shared by two blocks is finished IN ORDER (the second block starts from the first one's parked accumulators), so the
 * result is bit-identical to cmdiad_gemm_bf16's.  Takes the cmdiad_gemm_args of the residual form only (A, W, bias, residual,
 * out_f32; everything else unset).  workspace: cmdiad_gemm_streamk_workspace_bytes() bytes, ZERO-INITIALISED once by the caller
 * and then left to the library (slots + hand-over counters; the kernel leaves the counters at zero again).  ONE stream-K launch in
 * flight PER DEVICE, not only per workspace: block b spins on block b - 1's counter, which assumes its predecessor is resident or
 * will be dispatched -- two overlapping launches (two streams) can fill every CU with waiting blocks of both.  The caller orders
 * them (cmdiad_amd.ops.gemm_streamk: an event between consecutive launches on different streams).
 * cmdiad_gemm_streamk_eligible(M, N, K) -> 1 when the shape qualifies. */
size_t cmdiad_gemm_streamk_workspace_bytes(void);
int cmdiad_gemm_streamk_eligible(int M, int N, int K);
int cmdiad_gemm_streamk_bf16(const cmdiad_gemm_args* a, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* LayerNorm statistics from the producer's chunk partials (nn.LayerNorm inside Block, models/models.py:170,175): part
 * [chunks][M][2] as written through cmdiad_gemm_args.ln_part -> rstd[m] = 1 / sqrt(var_m + eps) over the chunks * 64 columns
 * (biased variance, as torch) and, optionally, mean_out[m].  Chunks are merged in order (Chan's formula): bit-reproducible. */
int cmdiad_ln_stats_finalize(const float* part, int M, int chunks, float eps, float* rstd, float* mean_out,
                             cmdiad_stream_t stream);

/* Weight-gradient product of the trainer (hallucination_network_pretrain.py:114-131, loss.backward() through
 * utils/utils.py:94-100): C[N1,N2] = sum_m P[m,n1] * Q[m,n2] with BOTH operands row-major bf16 (P = dZ [M,N1], Q = the
 * layer input [M,N2]) -- no transposed copies.  M % 64 == 0, N1 % 8 == 0, N2 % 8 == 0.  split_k > 1: grid.y slices of M, slab s
 * of out_f32 ([split_k][N1][ldo]) receives partial sum s (cmdiad_reduce_slabs adds them); every slab is fully written.
 * colsum_out (NULL allowed) [split_k][N1] f32: partial column sums of P, i.e. the bias gradient sum_m dZ[m, n1], from the
 * tiles already staged for the product. */
int cmdiad_gemm_tn_bf16(const uint16_t* P, int ldp, const uint16_t* Q, int ldq, int M, int N1, int N2, int split_k,
                        float* out_f32, int ldo, float* colsum_out, cmdiad_stream_t stream);

/* QKV projection with head-split stores for the attention kernel (models/models.py:150-151):
 * A [B*T, C] bf16, W [3C, C], bias [3C] or NULL.  head_dim = 64, C = H*64.
 * q_out, k_out [B,H,Tp,64] bf16 (q pre-multiplied by head_dim^-0.5 (models.py:153) times log2(e)),
 * vt_out [B,H,64,Tp] bf16 (V transposed); Tp = T rounded up to 64; padding is never written.
 * row_scale [B*T] f32 or NULL (ABI 3): qkv = row_scale[m] * (A . W^T) + bias, the consumer side of the LayerNorm fold
 * (cmdiad_gemm_args.row_scale). */
int cmdiad_gemm_qkv(const uint16_t* A, const uint16_t* W, const float* bias, const float* row_scale, int B, int T, int C,
                    uint16_t* q_out, uint16_t* k_out, uint16_t* vt_out, cmdiad_stream_t stream);

/* softmax(q k^T) v per (image, head) (models/models.py:153-157), flash-style, bf16 MFMA; q as written by
 * cmdiad_gemm_qkv (pre-scaled by head_dim^-0.5 * log2(e): the kernel evaluates exp2 of the raw q.k).
 * out [B*T, C] bf16 with heads concatenated along C (the `.transpose(1,2).reshape(B,N,C)` of :157).
 * Padding (rows / columns T .. Tp-1 of q, k [B,H,Tp,64] and vt [B,H,64,Tp], Tp = T rounded up to 64): keys at and beyond T
 * are masked, whatever finite values the k padding holds; q padding rows are computed and discarded; vt padding columns are
 * multiplied by exact zeros and must therefore be finite (0 x inf is NaN) -- the caller zeroes them once. */
int cmdiad_attention(const uint16_t* q, const uint16_t* k, const uint16_t* vt, int B, int H, int T,
                     uint16_t* out, cmdiad_stream_t stream);

/* y = LayerNorm(x (+ add)) * gamma + beta -> bf16; when `add` is given (Point-MAE re-adds the
 * positional embedding in front of every block, models/models.py:240) x is updated in place to
 * x + add first.  x [M,C] f32, add [M,C] f32 or NULL, C % 64 == 0, C <= 1024.
 * out_bf16 [M, C] (NULL allowed); out_f32 (NULL allowed) with leading dimension ldo32. */
int cmdiad_layernorm(float* x, const float* add, const float* gamma, const float* beta, float eps, int M,
                     int C, uint16_t* out_bf16, float* out_f32, int ldo32, float* mean_out, float* rstd_out,
                     cmdiad_stream_t stream);

/* LayerNorm of every row but the first of each of B segments of T rows (Point-BERT's fetch layers drop the cls row,
 * models/models.py:348): x [B*T, C] f32 -> out_f32 row b*(T-1) + t-1 (leading dimension ldo32) = LN(x row b*T + t), t >= 1.
 * Same arithmetic as cmdiad_layernorm's float2 form.  C % 128 == 0, 128 <= C <= 1024, T >= 2. */
int cmdiad_layernorm_skip_first(const float* x, const float* gamma, const float* beta, float eps, int B, int T, int C,
                                float* out_f32, int ldo32, cmdiad_stream_t stream);

/* Row b*T of x [B*T, C] <- lead_x [C] and of pos <- lead_pos [C] (pos and lead_pos: both or neither), for b < B: Point-BERT's cls
 * token and cls_pos (models/models.py:338-344) in front of each cloud's token rows. */
int cmdiad_lead_rows(float* x, float* pos, const float* lead_x, const float* lead_pos, int B, int T, int C, cmdiad_stream_t stream);

/* Second half of the Point-MAE encoder in one kernel (models/models.py:204-215): h3 = ReLU(W3b . h2 + gb[group]) is produced
 * and consumed in LDS, tok[g] = max over the group's rows of (W4 . h3 + b4).  h2 [groups*Mg, 256] bf16 and gb [groups, 512] f32
 * (= W3a . groupmax(h2) + b3) as produced by cmdiad_encoder_stage1 + cmdiad_gemm_bf16; W3b [512,256], W4 [384,512] bf16;
 * tok_out [groups, 384] f32.  Bit-identical to cmdiad_gemm_bf16(ReLU, group_bias) followed by cmdiad_gemm_groupmax. */
int cmdiad_encoder_tail(const uint16_t* h2, const float* gb, const uint16_t* W3b, const uint16_t* W4, const float* b4,
                        int groups, int Mg, float* tok_out, cmdiad_stream_t stream);

/* The same kernel at n_out output columns: 384 (= cmdiad_encoder_tail) or 256 (Point-BERT's encoder, models/models.py:31-33 with
 * encoder_dims = 256: W4 [256,512], b4 [256]).  seg = 0: tok_out [groups, n_out]; seg > 0 (n_out 256 only, seg | groups): group g's
 * token goes to row g + g / seg + 1 of tok_out [groups + groups / seg, n_out], i.e. every cloud of seg groups gets one leading row
 * that is NOT written (Point-BERT's cls row, filled after reduce_dim by cmdiad_lead_rows).  Bit-identical to
 * cmdiad_gemm_bf16(ReLU, group_bias) + cmdiad_gemm_groupmax at N = n_out. */
int cmdiad_encoder_tail_n(const uint16_t* h2, const float* gb, const uint16_t* W3b, const uint16_t* W4, const float* b4,
                          int groups, int Mg, int n_out, int seg, float* tok_out, cmdiad_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Convolution heads of the distillation networks: models/hallucination_network.py:72-143
 * (HallucinationCrossModalityConv), 146-182 (HallucinationRGBFeatureToXYZInputMLP), 185-220
 * (HallucinationFeatureToInputConv), models/hrnet.py:8-43,146-290 (HRNet stem + Bottlenecks).
 * Replaces the torch.nn.Conv2d / BatchNorm2d / interpolate calls those modules make (cuDNN in the reference).
 * ------------------------------------------------------------------------------------------- */

/* 3x3 (stride 1 or 2, padding 1) or 1x1 convolution as an implicit GEMM: x [B,H,W,C] bf16 NHWC (a token matrix
 * [B, H*W, C] is exactly that), W [N][ksize*ksize][C] bf16 (tap-major: the torch weight [N,C,kh,kw] permuted to
 * [N,kh,kw,C]; BatchNorm folded by the caller), C % 64 == 0, N % 4 == 0.  Output rows m = (b, yo, xo) with
 * Ho = (H + 2 pad - ksize) / stride + 1.  Epilogue: + bias[N]; ReLU (act = RELU); + residual[M,N] f32; ReLU
 * (act = RELU_POST); stores to out_f32 and/or out_bf16 with leading dimensions ldo32 / ldo16 (columns >= N untouched). */
typedef struct {
    const uint16_t* x; int B, H, Wd, C;
    const uint16_t* W; int N;
    int ksize, stride;
    const float* bias;               /* [N] or NULL */
    int act;                         /* CMDIAD_ACT_NONE / RELU / RELU_POST */
    const float* residual; int ldr;  /* [M,N] f32 or NULL */
    float* out_f32; int ldo32;
    uint16_t* out_bf16; int ldo16;
} cmdiad_conv_args;
int cmdiad_conv2d_nhwc_bf16(const cmdiad_conv_args* args, cmdiad_stream_t stream);

/* Stem convolution (hrnet.py:150-151,252-254): 3x3, padding 1, stride 1 or 2 on an f32 NCHW image with Cin <= 4 planes,
 * folded BatchNorm bias, ReLU, bf16 NHWC output [B,Ho,Wo,Cout].  w [Cout][Cin][3][3] f32 (torch layout), Cout % 8 == 0. */
int cmdiad_conv_stem(const float* x, const float* w, const float* bias, int B, int Cin, int H, int W, int Cout,
                     int stride, uint16_t* out, cmdiad_stream_t stream);

/* torch.nn.functional.interpolate(mode='bicubic', align_corners=False) (hallucination_network.py:171,204).
 * in f32 NHWC [B,h,w,ldi] of which C channels are used; exactly one output: out_bf16_nhwc [B,H,W,ldo] (the next
 * convolution's operand; columns >= C untouched) or out_f32_nchw [B,C,H,W]. */
int cmdiad_upsample_bicubic(const float* in, int B, int h, int w, int C, int ldi, int H, int W,
                            uint16_t* out_bf16_nhwc, int ldo, float* out_f32_nchw, cmdiad_stream_t stream);

/* One whole pre-LN transformer block on the fp32 residual stream x [B*T, C], in place (models/models.py:177-180 Block.forward,
 * 148-160 Attention, 126-132 Mlp; timm's ViT block reached at models.py:48 has the same algebra):
 *   x += proj(softmax(q k^T) v) with q,k,v = qkv(LN1(x (+ pos)));   x += fc2(GELU(fc1(LN2(x)))).
 * pos [B*T, C] f32 or NULL is added to x first (Point-MAE re-adds the positional embedding in front of every block,
 * models.py:240).  Weights: bf16 [out, in] matrices in nn.Linear layout, f32 biases / LayerNorm parameters (qkv_b may be
 * NULL).  C = 64 H.  q, k [B,H,Tp,64] and vt [B,H,64,Tp] bf16 scratch as in cmdiad_gemm_qkv (padding rows zeroed once by
 * the caller); workspace >= cmdiad_transformer_block_workspace_bytes(B*T, C, hidden).  Sequencing only: LayerNorm ->
 * cmdiad_gemm_qkv -> cmdiad_attention -> cmdiad_gemm_bf16 x3, all on `stream`.
 * ABI 3: with the folded weights present (qkv_wf ... fc1_bf: gamma o W centred over k as bf16, b + W beta; see
 * cmdiad_gemm_args.row_scale) the second LayerNorm is folded into proj (producer) and fc1 (consumer), and with
 *   CMDIAD_BLOCK_PREP_NEXT  fc2 also emits the bf16 rows + statistics of its output (+ pos: the NEXT block's input) into the
 *                           workspace, which the next call on the same workspace consumes when it is given
 *   CMDIAD_BLOCK_LN1_READY  (the first LayerNorm is folded into qkv; pos is NOT added again).
 * A block whose output is read before the next block (Point-MAE's fetch layers) is called without PREP_NEXT. */
typedef struct {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    const uint16_t* qkv_w; const float* qkv_b;
    const uint16_t* proj_w; const float* proj_b;
    const uint16_t* fc1_w; const float* fc1_b;
    const uint16_t* fc2_w; const float* fc2_b;
    const uint16_t* qkv_wf; const float* qkv_bf;   /* ABI 3: LayerNorm-folded qkv / fc1 (all four or none) */
    const uint16_t* fc1_wf; const float* fc1_bf;
} cmdiad_block_weights;
enum { CMDIAD_BLOCK_LN1_READY = 1, CMDIAD_BLOCK_PREP_NEXT = 2 };
size_t cmdiad_transformer_block_workspace_bytes(int M, int C, int hidden);
int cmdiad_transformer_block_fwd(float* x, const float* pos, const cmdiad_block_weights* w, int B, int T, int C, int H,
                                 int hidden, float eps, int flags, uint16_t* q, uint16_t* k, uint16_t* vt, void* workspace,
                                 size_t workspace_bytes, cmdiad_stream_t stream);

/* Point-MAE Encoder (models/models.py:200-215), eval-mode BatchNorm folded into the convolutions:
 *   h1 = relu(W1' x + b1')            3 -> 128   (computed on the fly while staging the GEMM tile)
 *   h2 = W2 h1 + b2                   128 -> 256 ; g = max over the group's points
 * neigh [groups*Mg, 3] f32; w1 [128,4] f32 = {w_x, w_y, w_z, b} per output channel (BN folded).
 * Writes h2 [groups*Mg, 256] bf16, gmax [groups, 256] f32 and (optional) its bf16 copy.
 * Mg (points per group) must be 128, 64 or 32. */
int cmdiad_encoder_stage1(const float* neigh, const float* w1, const uint16_t* W2, const float* b2,
                          int groups, int Mg, uint16_t* h2_out, float* gmax_out, uint16_t* gmax_bf16_out,
                          cmdiad_stream_t stream);
/* out[g][n] = max over the Mg rows of group g of (A . W^T + bias)[row][n]  (torch.max(...,dim=2),
 * models/models.py:214).  A [groups*Mg, K] bf16, W [N,K] bf16, out [groups, N] f32 and/or bf16. */
int cmdiad_gemm_groupmax(const uint16_t* A, const uint16_t* W, const float* bias, int groups, int Mg, int N,
                         int K, float* out_f32, uint16_t* out_bf16, cmdiad_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Patch-library nearest-neighbour scoring
 * ------------------------------------------------------------------------------------------- */

/* Per-query nearest bank row under L2 (torch.cdist + torch.min(dim=1), features.py:190,227) without
 * materialising the QxNb matrix: 16-bit MFMA distance GEMM whose accumulators start at -(|q|^2 + |b|^2) / 2, so that a
 * finished accumulator is -d2 / 2, with a running (min, argmin) epilogue.  keys[q] = min over rows of
 * ((fp32 bits of max(d2', 0)) << 32 | row_offset+row), d2' = d2 with the four low mantissa bits of -d2 / 2 cleared (the
 * epilogue carries the element's place there; 2^-19 of the value, three orders below the operand rounding):
 * integer order == (distance, index) order, so bank shards combine with an integer MIN (RCCL
 * all-reduce over xGMI) and ties resolve to the lowest global row, as torch.min does.  The key of a (query, row) pair does
 * not depend on the launch geometry, the tile shape or the shard the row is in.
 * q [Q,D] bf16, q_sqnorm [Q] f32, bank [Nb,D] bf16, bank_sqnorm [Nb] f32 (squared norms of the
 * bf16-rounded rows, from cmdiad_normalize_cast), keys [Q] u64: the caller initialises keys to
 * UINT64_MAX (or any value above every key, e.g. INT64_MAX); the kernel combines with atomic min.  D % 64 == 0.
 * keys2 [Q] u64 or NULL (ABI 6), initialised like keys: the RUNNER-UP of every query, so that the exact fp32 re-score
 * (cmdiad_l2_rescore2) can repair a near-tie that the 16-bit operands resolved the wrong way -- torch.min on the fp32 cdist
 * (features.py:227) is index work, and with it min_idx equals the fp32 argmin except where a THIRD row lies inside the operand
 * noise too.  Definition (library rows only -- no tile shape, launch geometry or shard in it): the library is cut into groups of
 * 16 rows, group(row) = (row >> 6, (row >> 2) & 3) on GLOBAL rows (row_offset % 64 == 0 is required with keys2); keys2[q] is the
 * smallest key among the group minima other than keys[q]'s own group, i.e. the nearest row outside the winner's group.  Shards
 * combine as: K1 = MIN over shards of keys; K2 = MIN over shards of (keys == K1 ? keys2 : keys).
 * Contract: operands and norms finite (cmdiad_normalize_cast guarantees it: a row with a non-finite element is stored as zeros
 * with squared norm +inf -- as a library row it can never win, as a query it finds nothing and its keys stay untouched). */
enum { CMDIAD_DT_BF16 = 0, CMDIAD_DT_F16 = 1 };   /* 16-bit operand type of the distance GEMM */
int cmdiad_l2_min_keys(const uint16_t* q, const float* q_sqnorm, const uint16_t* bank, const float* bank_sqnorm,
                       int Q, int Nb, int D, uint32_t row_offset, unsigned long long* keys, unsigned long long* keys2, int dtype,
                       cmdiad_stream_t stream);

/* The same search over a query set whose live row count is known only on the device (*q_count <= Q_max, e.g. the compacted set of
 * cmdiad_rows_dedup_plan): the launch is sized for Q_max, rows at and beyond *q_count are neither read nor written. */
int cmdiad_l2_min_keys_counted(const uint16_t* q, const float* q_sqnorm, const int* q_count, int Q_max, const uint16_t* bank,
                               const float* bank_sqnorm, int Nb, int D, uint32_t row_offset, unsigned long long* keys,
                               unsigned long long* keys2, int dtype, cmdiad_stream_t stream);

/* The same search over n_seg query SEGMENTS laid out at a fixed stride -- the row-sharded search of SURVEY 8(e): the gathered,
 * separately compacted query sets of the W ranks of a node against THIS rank's library shard (what features.py:186-190,227 do on
 * one device, per shard).  Segment w = rows [w * seg_stride, w * seg_stride + min(seg_counts[w], seg_stride)) of q / q_sqnorm /
 * keys ([n_seg * seg_stride] each); seg_counts [n_seg] int32 lives on the device, so no host read sizes the launch: ONE launch
 * walks the live query tiles of all segments as one tile list (XCD-aware mapping over the live blocks), instead of one launch per
 * segment.  1 <= n_seg <= 64. */
int cmdiad_l2_min_keys_segments(const uint16_t* q, const float* q_sqnorm, const int* seg_counts, int n_seg, int seg_stride,
                                const uint16_t* bank, const float* bank_sqnorm, int Nb, int D, uint32_t row_offset,
                                unsigned long long* keys, unsigned long long* keys2, int dtype, cmdiad_stream_t stream);

/* Exact removal of repeated query rows in front of the search.  Every patch of the 56 x 56 grid without a foreground pixel under
 * it is the same vector ((0 - mean) / std in every column; features.py:169-184, multiple_features.py:976-977) and the reference's
 * torch.cdist (features.py:186-190) searches the library again for each of them (likewise the hallucinated features of those
 * patches, multiple_features.py:351).  The MOST REPEATED row of the batch is found by a row hash; a row repeats its first
 * occurrence iff hash and squared-norm bits are equal AND all D elements compare equal -- then everything cmdiad_l2_min_keys reads
 * for it is identical and so is its key (a hash collision costs a comparison, never an answer).  slot[Q] (row of the compacted set
 * that answers for q), rows[Q] (compacted -> original, first *count entries), count[1], q_compact [Q,D] / q_sqnorm_compact [Q]
 * (first *count rows written), all on the device; workspace: cmdiad_rows_dedup_workspace_bytes(Q).  Order-preserving; a batch
 * without a repeated row compacts to itself. */
size_t cmdiad_rows_dedup_workspace_bytes(int Q);
int cmdiad_rows_dedup_plan(const uint16_t* q, const float* q_sqnorm, int Q, int D, void* workspace, int* slot, int* rows, int* count,
                           uint16_t* q_compact, float* q_sqnorm_compact, cmdiad_stream_t stream);
/* keys[q] = keys_compact[slot[q]] */
int cmdiad_keys_expand(const unsigned long long* keys_compact, const int* slot, int Q, unsigned long long* keys,
                       cmdiad_stream_t stream);
/* out[q, :] = rows_compact[slot[q], :] (f32, D % 4 == 0): the per-row results of a computation that ran on the compacted rows
 * only (the hallucination MLP of the MTFI path, hallucination_network.py:34-45), back on every original row. */
int cmdiad_rows_expand_f32(const float* rows_compact, const int* slot, int Q, int D, float* out, cmdiad_stream_t stream);

/* Exact fp32 re-score of the winners: min_val[q] = || q_f32[q] - bank_f32[idx - row_offset] ||_2,
 * min_idx[q] = idx (global row).  Queries whose winner lies outside [row_offset, row_offset+Nb) are
 * left untouched (another shard owns them). */
int cmdiad_l2_rescore(const float* q, const float* bank, const unsigned long long* keys, int Q, int Nb,
                      int D, uint32_t row_offset, float* min_val, int64_t* min_idx, cmdiad_stream_t stream);
/* The same over BOTH candidates of every query (keys = best, keys2 = runner-up of cmdiad_l2_min_keys): squared fp32 distances in
 * one summation order; the smaller one wins, of equal ones the lower row -- torch.min's answer on the fp32 distance matrix
 * (features.py:227) wherever the true nearest row is one of the two.
 *   min_val / min_idx (both or neither): the decision, written for queries whose best candidate lies in [row_offset, row_offset+Nb)
 *     (a runner-up outside that range is ignored: use d2_pair + cmdiad_l2_choose when the fp32 rows are sharded);
 *   d2_pair [2][Q] f32 or NULL: the squared distances of the candidates THIS shard owns, others untouched -- zero-filled by the
 *     caller and summed over the shards, every entry has exactly one contributor; cmdiad_l2_choose then takes the decision. */
int cmdiad_l2_rescore2(const float* q, const float* bank, const unsigned long long* keys, const unsigned long long* keys2, int Q,
                       int Nb, int D, uint32_t row_offset, float* d2_pair, float* min_val, int64_t* min_idx, cmdiad_stream_t stream);
int cmdiad_l2_choose(const unsigned long long* keys, const unsigned long long* keys2, const float* d2_pair, int Q, float* min_val,
                     int64_t* min_idx, cmdiad_stream_t stream);

/* Batch-statistics BatchNorm support (the reference runs Point-MAE's BatchNorm1d layers, models/models.py:189,195,
 * in training mode because the extractor is never put in .eval()).  Double-precision moment sums, ACCUMULATED into
 * caller-zeroed buffers:  col_moments: x [rows,C] f32 (row pitch ld) -> sum[C], sumsq[C];
 * moments3: xyz [rows,3] f32 -> out9 = (x, y, z, xx, xy, xz, yy, yz, zz) sums. */
int cmdiad_col_moments(const float* x, size_t rows, int C, int ld, double* sum, double* sumsq, cmdiad_stream_t stream);
int cmdiad_moments3(const float* xyz, size_t rows, double* out9, cmdiad_stream_t stream);

/* Library copy laid out for the fp32 matrix cores ("block16"): groups of 16 rows,
 * out[(((g * D/16 + t) * 4 + kq) * 16 + j) * 4 + e] = bank[16 g + j][16 t + 4 kq + e] (zero beyond Nb),
 * cmdiad_bank_block16_floats(Nb, D) = ceil(Nb/16) * 16 * D floats.  Built once per library; the re-weighting scan
 * streams it with fully coalesced 1 KiB loads straight into MFMA B operands. */
size_t cmdiad_bank_block16_floats(int Nb, int D);
int cmdiad_bank_block16(const float* bank, int Nb, int D, float* out, cmdiad_stream_t stream);

/* Re-weighting scan (features.py:235-254: torch.cdist(m_star, bank) + topk(3, largest=False)): for each of R <= 32
 * probe rows (m_star) the 3 nearest library rows as packed keys (EXACT fp32 squared distance bits << 32 | global row),
 * merged into top3 [R,3] u64, which the caller initialises to UINT64_MAX or 0x7FFF...F (shards call it in turn or
 * all-gather their top3).  One pass over bank_block16 for all probes (v_mfma_f32_16x16x4_f32 cross term, 8 approximate
 * candidates per probe), then the candidates are re-evaluated exactly on the row-major library.  ABI version 2: R <= 32 per
 * call (version 1 took 64) and a workspace of 8 candidates per probe and block (cmdiad_reweight_workspace_bytes).
 * probes [R,D] f32, bank [Nb,D] f32 row-major, bank_block16 from cmdiad_bank_block16; D % 128 == 0. */
size_t cmdiad_reweight_workspace_bytes(int R, int Nb);
int cmdiad_reweight_scan(const float* probes, const float* bank, const float* bank_block16, int R, int Nb, int D,
                         uint32_t row_offset, unsigned long long* top3, void* workspace, size_t workspace_bytes,
                         cmdiad_stream_t stream);
/* The same for the TWO libraries of a scored batch in one launch pair (features.py:235-254 runs per library: xyz and rgb / fusion,
 * multiple_features.py:976-1003): problem 0 and problem 1 each as in cmdiad_reweight_scan (own probes, library, row offset and
 * top3); the scan kernel's workgroups are shared between the libraries in proportion to their rows, so the small library's fixed
 * cost (probes into LDS, candidate merges, the exact re-evaluation launch) runs beside the large library's stream instead of after
 * it.  Results identical to two separate calls.  Both Nb > 0 (an empty shard takes the single-library call for the other). */
size_t cmdiad_reweight_pair_workspace_bytes(int Nb0, int Nb1);
int cmdiad_reweight_scan_pair(const float* probes0, const float* bank0, const float* bank0_block16, int R0, int Nb0,
                              uint32_t row_offset0, unsigned long long* top3_0, const float* probes1, const float* bank1,
                              const float* bank1_block16, int R1, int Nb1, uint32_t row_offset1, unsigned long long* top3_1,
                              int D, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* calculate_dist (features.py:186-190) as a MATERIALISED matrix, exact fp32 (sum of squared differences):
 * out[q][n] = || Q[q] - bank[n] ||_2, [Q, Nb] row-major.  API compatibility of DistHandle.materialize() only: the
 * scoring path never builds the Q x Nb matrix (960 MB per image at the reference's sizes). */
int cmdiad_l2_dist_matrix(const float* q, const float* bank, int Q, int Nb, int D, float* out, cmdiad_stream_t stream);

/* compute_single_s_s_map head / tail (features.py:227-290), batched over B images.
 * head: s_idx[b] = argmax_q min_val[b][q] (first occurrence), s_star[b] = the max; copies
 *       m_test[b] = patch[b][s_idx] and m_star[b] = bank[min_idx[b][s_idx] - row_offset] (only when that
 *       row lies in this shard) into [B,D] buffers (m_star feeds cmdiad_reweight_scan).
 * tail: knn_d[b][k-1] = || m_test[b] - bank[top3[b][k]] || for k = 1, 2 (rows owned by this shard only).
 * final: s[b] = (1 - exp(s_star / sqrt(D)) / sum_k exp(knn_d[b][k] / sqrt(D))) x s_star. */
int cmdiad_score_head(const float* min_val, const int64_t* min_idx, const float* patch, const float* bank,
                      int B, int Q, int D, int Nb, uint32_t row_offset, float* s_star, int32_t* s_idx,
                      float* m_test, float* m_star, cmdiad_stream_t stream);
int cmdiad_score_tail(const float* s_star, const float* m_test, const unsigned long long* top3,
                      const float* bank, int B, int D, int Nb, uint32_t row_offset, float* knn_d,
                      cmdiad_stream_t stream);
int cmdiad_score_final(const float* s_star, const float* knn_d, int B, int D, float* s_out,
                       cmdiad_stream_t stream);

/* Greedy k-centre coreset selection (features.py:372-425, get_coreset_idx_randomp after the random
 * projection; coreset_dtype 'FP16', dist_method_coreset 'l2').  z32 [n,d] f32 projected library (d even),
 * first_idx = 0 as the reference; idx_out [n_select] int64 in selection order. */
size_t cmdiad_coreset_workspace_bytes(int n, int d, int n_select);
int cmdiad_coreset_greedy(const float* z32, int n, int d, int n_select, int first_idx, int64_t* idx_out,
                          void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);
/* coreset_dtype 'TF32' (features.py:390-391; main.py:151): the same selection on the UNROUNDED fp32 rows -- allow_tf32 only touches
 * matrix products and the loop has none, so the reference's branch is an fp32 scan: dist = sqrt(sum (z_i - z_last)^2) in fp32, fp32
 * running minimum, first arg-max.  d <= 1024 (any parity). */
/* Row-sharded selection (fit-time sharding): every rank holds the projected library and scans its own row range; between
 * rounds the caller all-reduces (MAX) the 8-byte packed winner keys of the ranks.  prepare: the first pass (workspace:
 * cmdiad_coreset_workspace_bytes(n, d, 1)); round: rows [row_lo, row_hi) (row_lo % 4 == 0; row_hi % 4 == 0 or == n) against the pivot
 * named by *pivot_key (NULL: row first_idx), winner into *best_out with atomic max (the caller zeroes it first); decode: keys[r] of
 * rounds 0 .. n_select - 2 -> idx_out[0] = first_idx, idx_out[r + 1] = row of keys[r].  Picks identical to cmdiad_coreset_greedy. */
int cmdiad_coreset_prepare(const float* z32, int n, int d, int first_idx, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);
int cmdiad_coreset_round(void* workspace, int n, int d, int row_lo, int row_hi, const unsigned long long* pivot_key, int first_idx,
                         unsigned long long* best_out, cmdiad_stream_t stream);
int cmdiad_coreset_decode(const unsigned long long* keys, int n_select, int first_idx, int64_t* idx_out, cmdiad_stream_t stream);
size_t cmdiad_coreset_f32_workspace_bytes(int n, int d, int n_select);
int cmdiad_coreset_greedy_f32(const float* z32, int n, int d, int n_select, int first_idx, int64_t* idx_out, void* workspace,
                              size_t workspace_bytes, cmdiad_stream_t stream);

/* Sparse random projection in front of the coreset selection (features.py:360-371: SparseRandomProjection.fit_transform): out [n,
 * n_comp] = X [n,d] . components^T with `components` [n_comp,d] in CSR (int32 indptr / sorted indices, f32 data: the fitted
 * transformer's components_, ABI 3).  Per output element the products are added one by one in the order of the row's non-zeros,
 * each product and each sum rounded to float32 -- the arithmetic of the scipy routine sklearn calls, so out is bit-identical to the
 * host transform.  d <= 4096. */
int cmdiad_sparse_project_f32(const float* X, size_t n, int d, const int* indptr, const int* indices, const float* data, int n_comp,
                              float* out, cmdiad_stream_t stream);


/* ---------------------------------------------------------------------------------------------
 * Small fused element-wise / layout kernels
 * ------------------------------------------------------------------------------------------- */

/* out_bf16 = bf16 or (out_dtype = CMDIAD_DT_F16) saturating fp16 of ((x - mean) * inv_std); optional out_f32 copy of the normalised values and
 * optional per-row squared norm of the bf16-rounded row (a11 + the |b|^2 term of the distance GEMM). */
int cmdiad_normalize_cast(const float* x, size_t rows, int D, float mean, float inv_std, uint16_t* out_bf16,
                          float* out_f32, float* row_sqnorm, int out_dtype, cmdiad_stream_t stream);
/* The same with the input rows in groups of group_rows, each preceded by group_skip rows that are NOT taken (ABI 6): output row r
 * reads input row r + (r / group_rows + 1) * group_skip.  The rgb patch features are rows 1..784 of every image's 785 ViT tokens
 * (features.py:160-162 drops the cls token, multiple_features.py:976-977 normalises): group_rows 784, group_skip 1 reads the
 * token tensor in place and writes the patch rows compactly.  A non-finite row: see cmdiad_l2_min_keys. */
int cmdiad_normalize_cast_rows(const float* x, size_t rows, int D, int group_rows, int group_skip, float mean, float inv_std,
                               uint16_t* out_bf16, float* out_f32, float* row_sqnorm, int out_dtype, cmdiad_stream_t stream);

/* ViT patch embedding as a GEMM operand: rgb [B,3,S,S] f32 -> patches [B*(S/8)^2, 192] bf16 with
 * k = (c, dy, dx) matching conv weight [768,3,8,8] flattened (timm PatchEmbed, models/models.py:41). */
int cmdiad_im2col_patch8(const float* rgb, int B, int S, uint16_t* patches, cmdiad_stream_t stream);
/* DINOv2 ViT-B/14 patch embedding as a GEMM operand (ABI 6, additive): rgb [B,3,S,S] f32, S % 14 == 0 (518 for
 * vit_base_patch14_dinov2.lvd142m) -> patches [B*(S/14)^2, 640] bf16, column k = c*196 + dy*14 + dx (conv weight [768,3,14,14]
 * flattened), columns 588..639 zero (the packed patch weight carries the same zero columns: K % 64 == 0). */
int cmdiad_im2col_patch14(const float* rgb, int B, int S, uint16_t* patches, cmdiad_stream_t stream);
/* AdaptiveAvgPool2d((56, 56)) of the patch-token grid (features.py:165-166, `rgb_patch2`), ABI 6, additive: tokens [B, 1 + s*s, C]
 * f32 read in place (the cls row of every image skipped), s x s row-major grid -> out [B, 3136, C] f32.  Windows
 * [floor(i s / 56), ceil((i + 1) s / 56)) per axis, summed from 0 in row-major order, divided by the window height and then by its
 * width, as ATen's CPU kernel does: the output equals torch.nn.functional.adaptive_avg_pool2d on the CPU BIT FOR BIT (at s = 28
 * every window is one cell: the exact 2x replication).  0 < s <= 1024, C % 4 == 0, 16-byte aligned buffers. */
int cmdiad_token_pool56(const float* tokens, int B, int s, int C, float* out, cmdiad_stream_t stream);
/* 3 x 3 im2col with padding 1 and stride 1 | 2 (hrnet.py:152, the trunk's stem convolution as a GEMM in the hand-written training
 * step): img [B,C,H,W] f32 -> cols [B*Ho*Wo, ld] bf16, column c * 9 + ky * 3 + kx (the order of the flattened Conv2d weight and of
 * torch.nn.functional.unfold), columns 9 C .. ld - 1 zero.  ld % 8 == 0, ld >= 9 C. */
int cmdiad_im2col3x3_bf16(const float* img, int B, int C, int H, int W, int stride, int ld, uint16_t* cols, cmdiad_stream_t stream);

/* tokens[b][0] = cls + pos[0]; tokens[b][1+i] = patch_out[b][i] + pos[1+i]  (timm _pos_embed,
 * models/models.py:42).  patch_out [B*P, C] f32, tokens [B*(P+1), C] f32. */
int cmdiad_vit_assemble(const float* patch_out, const float* cls, const float* pos, int B, int P, int C,
                        float* tokens, cmdiad_stream_t stream);

/* out[m][:] = act(W x[m] + b) for 3-d inputs: Point-MAE pos_embed first layer nn.Linear(3,128)+GELU
 * (models/models.py:268-272).  x [M,3] f32, wb [N,4] f32 = {w_x,w_y,w_z,bias}, out [M,N] bf16, N % 8 == 0. */
int cmdiad_linear3(const float* x, const float* wb, size_t M, int N, int act, uint16_t* out,
                   cmdiad_stream_t stream);

/* Bilinear up-sampling h x h -> H x H, align_corners=False (features.py:294). in [B,h,h], out [B,H,H]. */
int cmdiad_bilinear_up(const float* in, int B, int h, int H, float* out, cmdiad_stream_t stream);

/* ---- rest of the pointnet2_ops surface (the reference imports the package at models/models.py:5 but
 * only calls furthest_point_sample and gather_operation) ---- */

/* pointnet2_utils.ball_query(radius, nsample, xyz[B,N,3], new_xyz[B,M,3]) -> idx int32 [B,M,nsample]: the first nsample
 * points in index order with squared distance < radius^2, the first hit pre-filling every slot, zeros when nothing is in
 * range.  n_valid as in cmdiad_fps (NULL = N).  Bit-exact with oracle orc_ball_query. */
int cmdiad_ball_query(const float* xyz, const int32_t* n_valid, const float* new_xyz, int B, int N, int M, float radius,
                      int nsample, int32_t* idx_out, cmdiad_stream_t stream);

/* out[b,c,j] = feat[b,c,idx[b,j]]: pointnet2_utils.gather_operation (feat [B,C,N], idx [B,M] -> [B,C,M], models/models.py:77)
 * and grouping_operation (idx [B,M,nsample] flattened to J = M*nsample -> [B,C,M,nsample]).  idx int32, feat / out f32. */
int cmdiad_gather_points(const float* feat, const int32_t* idx, int B, int C, int N, int J, float* out, cmdiad_stream_t stream);

/* ---- on-device tail of the scorer ---- */

/* KNNGaussianBlur (utils/utils.py:71-83) for n_maps maps [n_maps,H,W] f32: each map is divided by its maximum, quantised
 * like torchvision's ToPILImage (mul(255).byte()), blurred exactly as Pillow's ImageFilter.GaussianBlur(radius) does on an
 * 8-bit image (three extended-box passes per axis, 2^24 fixed point; bit-exact with oracle orc_pil_gaussian_blur_u8),
 * and mapped back (/255 * max).  H, W >= 2*floor(box radius)+2, and two copies of the padded 8-bit image (in the larger of its
 * two orientations: cmdiad_blur8_lds_bytes) must fit the LDS: squares up to 284 x 284, narrow strips with a longer side. */
int cmdiad_blur8_maps(const float* maps, int n_maps, int H, int W, float radius, float* out, cmdiad_stream_t stream);
size_t cmdiad_blur8_lds_bytes(int H, int W);

/* Per-pixel late fusion (multiple_features.py:985-992: lambda-weighted map pairs -> seg_fuser.score_samples):
 * out[b,p] = ((sum_k double(float(lambdas[k] * maps[b,k,p])) * coef[k]) - offset) + offset, i.e. sklearn's
 * SGDOneClassSVM.score_samples for a model fitted on the host.  maps [B,K,HW] f32 (device), lambdas [K] and coef [K]
 * host arrays, 1 <= K <= 4, out [B,HW] f64 (device). */
int cmdiad_ocsvm_score_maps(const float* maps, int B, int K, int HW, const float* lambdas, const double* coef, double offset,
                            double* out, cmdiad_stream_t stream);

/* One-class SVM FIT on the device: scikit-learn's SGDOneClassSVM.fit for float32 inputs (feature_extractors/features.py:352-358,
 * detect_fuser.fit / seg_fuser.fit; algorithm of the reference's dependency: sklearn _sgd_fast._plain_sgd32 with hinge loss, L2
 * penalty alpha = nu / 2, 'optimal' schedule, shuffle = True, tol / n_iter_no_change stopping) with the same update order:
 * coef, offset and n_iter are those of scikit-learn (tests/test_gpu_ocsvm.py).  X [n,F] f32 on the device, 1 <= F <= 4;
 * seed = the 32-bit seed scikit-learn draws from random_state; pow2 [32][32] (host): column b of M^(2^e) of the xorshift32 step
 * (cmdiad_amd/ocsvm.py computes it); coef_out [F], offset_out, n_iter_out on the host.  Synchronous (one host decision per epoch). */
size_t cmdiad_ocsvm_fit_workspace_bytes(int n, int F);
int cmdiad_ocsvm_fit(const float* X, int n, int F, double nu, int max_iter, double tol, int n_iter_no_change, uint32_t seed,
                     const uint32_t* pow2, float* coef_out, double* offset_out, int* n_iter_out, void* workspace,
                     size_t workspace_bytes, cmdiad_stream_t stream);

/* ---- training side of the FtoF distillation network (models/hallucination_network.py:47-69,
 * hallucination_network_pretrain.py:102-159) ---- */

/* Loss head: y = GELU(z3); mode 0 'l2' sum_rows ||y-t||_2, 1 'cos_dist' sum_rows (1 - cos(y,t)), 2 'smooth_l1'
 * sum of elements (beta 1); row_loss [M] gets the per-row terms (reduce with cmdiad_sum_vector, scale 1/B);
 * dz3 [M,D] bf16 (NULL allowed) = inv_b * dLoss/dz3 (through the output GELU); y_out [M,D] f32 optional.
 * ABI 3: mode + CMDIAD_LOSS_OUT_NONE = no output activation (y = z3), mode + CMDIAD_LOSS_OUT_SIGMOID = sigmoid of the output AND
 * of the target -- the convolutional head's two losses (hallucination_network.py:136-147). */
enum { CMDIAD_LOSS_OUT_NONE = 256, CMDIAD_LOSS_OUT_SIGMOID = 512 };
int cmdiad_loss_head(const float* z3, const float* target, int M, int D, int mode, float inv_b,
                     float* row_loss, uint16_t* dz3, float* y_out, cmdiad_stream_t stream);

/* ---- training side of the convolutional FtoF head (models/hallucination_network.py:72-147: conv3x3 -> BatchNorm2d -> ReLU x3,
 * conv3x3 per direction; hallucination_network_pretrain.py:106-147 trains it in train() mode = BatchNorm on batch statistics).
 * Activations are NHWC flattened to [M = B*H*W, C].  Convolution forward and data gradient: cmdiad_conv2d_nhwc_bf16 (the latter on
 * flipped, transposed weights); weight gradient: cmdiad_gemm_tn_bf16 per filter tap over cmdiad_pad_nhwc_bf16 copies. ---- */

/* The constants of one batch-statistics BatchNorm from the float64 column sums of cmdiad_col_moments (sum, sumsq [C]) over `rows`
 * rows: mean64 / var64 [C] (biased variance; the caller's running-statistics update), scale = gamma / sqrt(var + eps),
 * shift = beta - mean * scale, mean, rstd as f32 [C]. */
int cmdiad_bn_affine(const double* sum, const double* sumsq, const float* gamma, const float* beta, size_t rows, double eps, int C,
                     double* mean64, double* var64, float* scale, float* shift, float* mean, float* rstd, cmdiad_stream_t stream);
/* y = z * scale[c] + shift[c] (+ residual [M,C] f32) (ReLU when relu != 0) as bf16 and / or f32 (NULL = not wanted): BatchNorm
 * (scale = gamma / sqrt(var + eps), shift = beta - mean * scale, batch statistics from cmdiad_col_moments) + ReLU,
 * nn.Sequential(..., BatchNorm2d, ReLU, ...) of hallucination_network.py:80-90; with the residual: bn3 + identity + ReLU of
 * Bottleneck.forward (hrnet.py:38-42).  C % 8 == 0. */
int cmdiad_bn_relu_fwd(const float* z, const float* scale, const float* shift, const float* residual, int relu, size_t M, int C,
                       uint16_t* y, float* y_f32, cmdiad_stream_t stream);
/* Backward of the same (autograd of hallucination_network_pretrain.py:146): with g = dy where z * scale + shift > 0 else 0
 * (masked != 0: the layer's own ReLU) or g = dy (masked == 0: no ReLU of its own -- the caller has applied the mask of the
 * ReLU after the residual sum) and xhat = (z - mean) * rstd:  part_dbeta / part_dgamma [chunks][C] = column sums of g /
 * g * xhat over `chunks` row ranges; cmdiad_bn_partials_sum adds them (fixed order) into dbeta / dgamma [C]; then
 * dz = scale * (g - dbeta / M - xhat * dgamma / M) as bf16 (per-channel vectors 16-byte aligned, C % 4 == 0). */
int cmdiad_bn_relu_bwd_reduce(const float* dy, const float* z, const float* scale, const float* shift, const float* mean,
                              const float* rstd, int masked, size_t M, int C, int chunks, float* part_dbeta, float* part_dgamma,
                              cmdiad_stream_t stream);
int cmdiad_bn_partials_sum(const float* part_dbeta, const float* part_dgamma, int chunks, int C, float* dbeta, float* dgamma,
                           cmdiad_stream_t stream);
int cmdiad_bn_relu_bwd_apply(const float* dy, const float* z, const float* scale, const float* shift, const float* mean,
                             const float* rstd, const float* dbeta, const float* dgamma, int masked, size_t M, int C, uint16_t* dz,
                             cmdiad_stream_t stream);
/* x [B,H,W,C] bf16 -> the interior of out [B,H+2,W+2,C] (border untouched: the caller zero-fills out once).  In that layout the
 * (ky, kx) tap of a 3x3 convolution with padding 1 is the row offset (ky-1)*(W+2) + (kx-1): the weight gradient of a tap is
 * one [M',N]^T [M',C] product of the padded output gradient with the shifted padded input.  C % 8 == 0. */
int cmdiad_pad_nhwc_bf16(const uint16_t* x, int B, int H, int W, int C, uint16_t* out, cmdiad_stream_t stream);
/* Backward pieces of the feature-to-input convolutional head (hallucination_network.py:185-220; trained by
 * hallucination_network_pretrain.py:106-147).  relu_bwd: dz = dx where the saved ReLU OUTPUT y (bf16) is positive, else 0, as bf16
 * and / or f32 (n elements, n % 4 == 0).  upsample_bicubic_bwd: adjoint of F.interpolate(mode='bicubic', align_corners=False) (:204):
 * grad_out f32 NHWC [B,H,W,C] -> grad_in f32 [B,h,w,C]; tmp f32 [B,H,w,C]; gathering passes, no atomics.  C % 4 == 0. */
int cmdiad_relu_bwd_bf16(const float* dx, const uint16_t* y, size_t n, uint16_t* dz, float* dz_f32, cmdiad_stream_t stream);
int cmdiad_upsample_bicubic_bwd(const float* grad_out, int B, int H, int W, int C, int h, int w, float* tmp, float* grad_in,
                                cmdiad_stream_t stream);


/* out[i] = scale * sum_s slabs[s*stride + i] in fixed order (split-K partials, column partials). n, stride % 4 == 0 */
int cmdiad_reduce_slabs(const float* slabs, int S, size_t n, size_t stride, float scale, float* out,
                        cmdiad_stream_t stream);
int cmdiad_sum_vector(const float* x, size_t n, float scale, float* out, cmdiad_stream_t stream);
/* partial[chunk][n] = sum over the chunk's rows of x[r][n]  (bias gradients). */
int cmdiad_colsum_bf16(const uint16_t* x, int M, int N, int chunks, float* partial, cmdiad_stream_t stream);
/* LayerNorm weight / bias gradient partials from dh [M,C], the LN input x and its saved row statistics. */
int cmdiad_ln_param_grad(const float* dh, const float* x, const float* mean, const float* rstd, int M, int C,
                         int chunks, float* partial_g, float* partial_b, cmdiad_stream_t stream);
/* torch.optim.Adam update (no weight decay, amsgrad off; hallucination_network_pretrain.py:261) on g*grad_scale;
 * optionally refreshes the bf16 GEMM operand copy of the parameter. */
int cmdiad_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                     float eps, int step, float grad_scale, uint16_t* p_bf16, cmdiad_stream_t stream);
/* The same update over a FLAT ARENA in one launch (additive, the ABI stays 6): p, g, m, v hold every parameter of a module one after
 * the other, each padded to a multiple of 4 floats (cmdiad_amd/dp_train.py: ParamArena), n % 4 == 0, all four 16-byte aligned
 * (p_bf16, optional: 8).  Element for element the arithmetic of cmdiad_adam_step: given equal inputs the results are bit-identical
 * to per-parameter calls.  A padding lane (g = m = v = 0) is left unchanged.  The grid is sized from the device's compute-unit
 * count (capped), not from n.  Null pointers, n % 4 != 0 and step < 1 are rejected before any launch. */
int cmdiad_adam_flat(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                     float eps, int step, float grad_scale, uint16_t* p_bf16, cmdiad_stream_t stream);

/* Generic fp32 -> bf16 cast (n % 4 == 0) and bf16 2-D transpose out[c][r] = in[r][c]. */
int cmdiad_cast_bf16(const float* x, size_t n, uint16_t* out, cmdiad_stream_t stream);
int cmdiad_transpose_bf16(const uint16_t* in, int rows, int cols, uint16_t* out, cmdiad_stream_t stream);

/* ---- scan preprocessing (utils/preprocessing.py:30-92: the reference calls open3d's segment_plane and cluster_dbscan; the
 * contract of both stages is this project's own, docs/preprocessing.md; additions are backwards compatible, the ABI stays 6) ---- */

/* RANSAC plane of `points` [E,3] f32: `iterations` hypotheses, hypothesis h fits the least-squares plane (float64) of n distinct
 * points drawn from a counter-based hash of (seed, h, draw counter); inliers: |a x + b y + c z + d| < distance_threshold in
 * float64; the winner has the most inliers (ties: the lowest h) and is refitted over all its inliers.
 * plane_out [4] f64 (device): unit normal with c >= 0, and d; info_out [2] int32 (device): {inliers of the winner, winner h}.
 * 3 <= n <= 64, n <= E.  workspace: cmdiad_plane_ransac_workspace_bytes(iterations). */
size_t cmdiad_plane_ransac_workspace_bytes(int iterations);
int cmdiad_plane_ransac(const float* points, int E, int n, int iterations, double distance_threshold, uint32_t seed,
                        double* plane_out, int32_t* info_out, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* remove_plane (utils/preprocessing.py:46-50), in place: pc [n_points,3] f32 and rgb [n_points, rgb_bytes] bytes (NULL with
 * rgb_bytes = 0: xyz only) are zeroed where |plane . (x, y, z, 1)| < distance_threshold (float64, strict).  plane [4] f64 (device). */
int cmdiad_plane_mask(float* pc, uint8_t* rgb, size_t n_points, int rgb_bytes, const double* plane, double distance_threshold,
                      cmdiad_stream_t stream);

/* DBSCAN labels of points [N,3] f32 (cluster_dbscan at utils/preprocessing.py:67; the labels are scikit-learn's): neighbours iff
 * dx^2 + dy^2 + dz^2 <= eps^2 in float64, core iff >= min_points neighbours counting itself, clusters = connected components of
 * the core points, numbered 0, 1, ... by their lowest core index; a non-core point with core neighbours takes the lowest cluster
 * number among them; everything else is -1.  labels [N] int32, n_clusters [1] int32 (both device).  N <= 2^24. */
size_t cmdiad_dbscan_workspace_bytes(int N);
int cmdiad_dbscan(const float* points, int N, double eps, int min_points, int32_t* labels, int32_t* n_clusters,
                  void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* hist[b] = number of labels equal to b - 1, b in [0, bins): bin 0 counts the noise label -1.  hist [bins] int32 (device). */
int cmdiad_label_histogram(const int32_t* labels, int N, int32_t* hist, int bins, cmdiad_stream_t stream);

/* The valid points of a scan as a STABLE compaction (valid: all three coordinates != 0 under numpy's rule: -0.0 is a zero, NaN is
 * not).  pc [H,W,3] f32 with `pitch` floats from one row to the next (>= 3 W: the window of a larger buffer can be read in place).
 * scan_edges: the sequence is get_edges_of_pc's (utils/preprocessing.py:20-27) -- rows 0 .. min(10,H) - 1 row-major, rows
 * max(H-10,0) .. H - 1, for every row the columns 0 .. min(10,W) - 1, for every row the columns max(W-10,0) .. W - 1; the corner blocks
 * appear twice.  scan_compact: all H * W pixels in raster order (np.nonzero(np.all(pc != 0, axis=1))), with index [.] int32 = the flat
 * pixel r * W + c of every kept point.  points [cap,3] f32; count [1] int32 = all valid points of the sequence, also when cap is
 * smaller (nothing is written past cap).  The output order is the sequence order: no atomic decides a position.  Sides in 1..16384,
 * H * W <= 2^26.  workspace: the size query of the same name. */
size_t cmdiad_scan_edges_workspace_bytes(int H, int W);
int cmdiad_scan_edges(const float* pc, size_t pitch, int H, int W, float* points, int cap, int32_t* count, void* workspace,
                      size_t workspace_bytes, cmdiad_stream_t stream);
size_t cmdiad_scan_compact_workspace_bytes(int H, int W);
int cmdiad_scan_compact(const float* pc, size_t pitch, int H, int W, float* points, int32_t* index, int cap, int32_t* count,
                        void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* connected_components_cleaning's decision and zeroing (utils/preprocessing.py:70-90) without the host: winner_out [1] int32 = (the
 * first maximum of hist[0 .. n_clusters]) - 1 -- bin 0 is the noise label -1, noise can win, ties go to the lowest bin: np.unique +
 * argmax --, then pc [n_pixels,3] f32 and rgb [n_pixels, rgb_bytes] bytes (NULL with rgb_bytes = 0) are zeroed at index[i] wherever
 * labels[i] != winner.  labels, index [N] int32; hist [bins] int32 (cmdiad_label_histogram; bins > n_clusters, else the bins that
 * are there compete); n_clusters [1] int32.  All device memory.  An index outside 0 .. n_pixels - 1 is skipped.  N = 0: nothing. */
int cmdiad_keep_largest_cluster(const int32_t* labels, const int32_t* index, int N, const int32_t* hist, int bins,
                                const int32_t* n_clusters, float* pc, uint8_t* rgb, size_t n_pixels, int rgb_bytes, int32_t* winner_out,
                                cmdiad_stream_t stream);

/* ---- sample preparation (dataset.py:62-65, 103-113, 168-171, 225-244: PIL + torchvision + numpy per sample on DataLoader workers;
 * contract: docs/sample_prep.md; additions are backwards compatible, the ABI stays 6).  All index and coefficient tables are device
 * arrays the caller computes on the host (cmdiad_amd/dataset.py); the kernels clamp every table entry to the source image. ---- */

/* Image.resize((out_w, out_h), BICUBIC) of B equal-sized images src [B,H,W,3] u8, bit for bit Pillow's 8-bit arithmetic: horizontal
 * pass into the 8-bit intermediate tmp [B,H,out_w,3], then the vertical pass; a pass whose side does not change is skipped (its
 * tables may be NULL; tmp may be NULL unless both sides change).  hcoef [out_w,hksize] / vcoef [out_h,vksize] int32: coefficients
 * with 22 fractional bits; hbounds [out_w,2] / vbounds [out_h,2] int32: (first source index, number of taps <= ksize).
 * out_u8 [B,out_h,out_w,3] (NULL allowed) and out_f32 [B,3,out_h,out_w] = norm[c*256 + value] (NULL allowed; norm [3,256] f32 is
 * ToTensor + Normalize as a table); at least one of the two. */
int cmdiad_resize_bicubic_u8(const uint8_t* src, int B, int H, int W, int out_h, int out_w, const int32_t* hcoef,
                             const int32_t* hbounds, int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize,
                             uint8_t* tmp, const float* norm, uint8_t* out_u8, float* out_f32, cmdiad_stream_t stream);

/* Organised cloud pc [B,H,W,3] f32 -> cloud_out [B,3,xyz_size,xyz_size] = pc[xyz_rows[y], xyz_cols[x]] (resize_organized_pc,
 * utils/mvtec3d_util.py:14-22), depth_out [B,3,depth_size,depth_size] = the z channel at (depth_rows[y], depth_cols[x]) three times
 * (dataset.py:108-109; NULL: not wanted), count_out [B] int32 = resized pixels whose three coordinates are all non-zero. */
int cmdiad_organized_pc_prep(const float* pc, int B, int H, int W, const int32_t* xyz_rows, const int32_t* xyz_cols, int xyz_size,
                             const int32_t* depth_rows, const int32_t* depth_cols, int depth_size, float* cloud_out,
                             float* depth_out, int32_t* count_out, cmdiad_stream_t stream);

/* Ground-truth mask gt [B,H,W] u8 -> out [B,1,gt_size,gt_size] f32 = 1.0 where gt[rows[y], cols[x]] / 255 > 0.5, else 0.0
 * (dataset.py:168-171, 239-241; rows / cols: Pillow's NEAREST rule). */
int cmdiad_gt_mask_prep(const uint8_t* gt, int B, int H, int W, const int32_t* rows, const int32_t* cols, int gt_size, float* out,
                        cmdiad_stream_t stream);

/* cmdiad_organized_pc_prep for a float64 cloud pc [B,H,W,3] (the Eyecandies tiffs of the reference's script): every gathered value
 * is converted to float32, round to nearest, as the reference's .float(); the valid-point rule is evaluated on the converted
 * values, as the float32 entry point evaluates it. */
int cmdiad_organized_pc_prep_f64(const double* pc, int B, int H, int W, const int32_t* xyz_rows, const int32_t* xyz_cols, int xyz_size,
                                 const int32_t* depth_rows, const int32_t* depth_cols, int depth_size, float* cloud_out,
                                 float* depth_out, int32_t* count_out, cmdiad_stream_t stream);

/* ---- Eyecandies: depth map -> organised cloud (utils/preprocessing_eyecandies.py:16-89; contract and operation order:
 * docs/eyecandies.md; additions are backwards compatible, the ABI stays 6) ---- */

/* One scan's parameters (device memory, 136 bytes): range = float32(maxd - mind) and mind = float32(mind) of *_info_depth.yaml,
 * inv_p = numpy.linalg.inv(K4 @ pose), row-major, computed on the host by the reference's own two numpy calls. */
typedef struct {
    float range;
    float mind;
    double inv_p[16];
} cmdiad_eyecandies_params;

/* depth_u16 [B,H,W] (the 16-bit PNG codes) -> cloud_out [B,H,W,3] f64 = remove_point_cloud_background(depth_to_pointcloud(...)) in
 * the reference's final layout and scale; removed_out [B,H,W] u8 = 1 where the background rule fired (NULL: not wanted);
 * depth_out [B,H,W] f32 = load_and_convert_depth (NULL: not wanted).  A removed point is the collapsed point of the reference, not
 * zero.  One launch, no synchronisation.  B in 1..65535, sides in 1..16384, H * W >= 513 (the anchors are the points at flat indices
 * 256 and H * W - 256). */
int cmdiad_eyecandies_cloud(const uint16_t* depth_u16, const cmdiad_eyecandies_params* params, int B, int H, int W,
                            double* cloud_out, uint8_t* removed_out, float* depth_out, cmdiad_stream_t stream);

/* The first stage alone: points_out [B,H*W,3] f64 = depth_to_pointcloud (NULL allowed), depth_out [B,H,W] f32 (NULL allowed); at
 * least one of the two. */
int cmdiad_eyecandies_unproject(const uint16_t* depth_u16, const cmdiad_eyecandies_params* params, int B, int H, int W,
                                double* points_out, float* depth_out, cmdiad_stream_t stream);

/* The second stage alone on any cloud: points [n,3] f64 -> cloud_out [n,3] f64 = remove_point_cloud_background(points),
 * removed_out [n] u8 (NULL allowed).  513 <= n <= 2^28. */
int cmdiad_eyecandies_background(const double* points, int n, double* cloud_out, uint8_t* removed_out, cmdiad_stream_t stream);

/* ---- pixel-level metrics: P-AUROC and AU-PRO (feature_extractors/features.py:302-324, utils/au_pro_util.py; contracts, the key
 * transform and the edge cases: docs/metrics.md; additions are backwards compatible, the ABI stays 6).  Every result is an integer
 * or a set whose order is not defined, so nothing depends on the order in which atomics arrive; the float64 arithmetic of the
 * metrics stays with the caller.  Everywhere: a negative size is rejected, size 0 returns CMDIAD_OK without a launch (the counters
 * and flag words that are passed are still zeroed), list lengths and n * H * W are at most 2^30. ---- */

/* 8-connected components of n masks [n,H,W], float32 or uint8 (mask_is_u8 = 0 / 1); foreground = value != 0.
 * labels [n,H,W] int32: 0 = background, 1 .. n_comp[i] = the components of image i numbered in raster order of their first pixel
 * (the numbering of scipy.ndimage.label with a 3 x 3 structure of ones); n_comp [n]; comp_offset [n + 1] = exclusive sum of n_comp
 * (comp_offset[n] = all components: the global id of a component is comp_offset[i] + label - 1); comp_size [comp_cap] int32 = pixels
 * per global id, zero past the last one; comp_cap >= n * ceil(H/2) * ceil(W/2), the most there can be.  nonbinary [1] int32 (NULL:
 * not wanted) = mask values that are neither 0 nor 1.  n in 0..65535, H, W >= 1, H * W <= 2^24. */
size_t cmdiad_ccl_workspace_bytes(int n, int H, int W);
int cmdiad_ccl_label(const void* masks, int mask_is_u8, int n, int H, int W, int32_t* labels, int32_t* n_comp, int32_t* comp_offset,
                     int32_t* comp_size, int comp_cap, int32_t* nonbinary, void* workspace, size_t workspace_bytes,
                     cmdiad_stream_t stream);

/* keys[i] = the bits of x[i] with -0.0 taken as +0.0, all flipped for a negative, the sign bit flipped otherwise: the unsigned order
 * of the keys is the order of the doubles.  nonfinite [1] int32 (NULL: not wanted) = NaN and infinite inputs.  The second is the
 * inverse map. */
int cmdiad_f64_to_keys(const double* x, int n, uint64_t* keys, int32_t* nonfinite, cmdiad_stream_t stream);
int cmdiad_keys_to_f64(const uint64_t* keys, int n, double* out, cmdiad_stream_t stream);

/* keys [n] sorted ascending in place (LSD radix, 8 passes of 8 bits, keys only; the workspace holds the second copy).  The tile
 * query returns the keys per block of a pass: sizes around its multiples are where the passes change shape. */
size_t cmdiad_sort_u64_tile(void);
size_t cmdiad_sort_u64_workspace_bytes(int n);
int cmdiad_sort_u64(uint64_t* keys, int n, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* preds [n,HW] f64 and the labels / comp_offset of the labelling -> ok_keys: the keys of the pixels with label 0; (def_score,
 * def_comp): score and global component id of every other pixel; counts [2] u64 = lengths of the two lists.  The order inside a list
 * is not defined.  Nothing is written past ok_cap / def_cap entries (counts still has the true lengths).  nonfinite as above. */
int cmdiad_metrics_split(const double* preds, const int32_t* labels, const int32_t* comp_offset, int n, int HW, uint64_t* ok_keys,
                         int ok_cap, double* def_score, int32_t* def_comp, int def_cap, uint64_t* counts, int32_t* nonfinite,
                         cmdiad_stream_t stream);

/* S [1] u64 = sum over the defect scores s of #(ok < s) + #(ok <= s), ok_sorted_keys [n_ok] = the sorted keys of the defect-free
 * scores (comparing keys is comparing the doubles): P-AUROC = S / (2 n_ok n_def). */
int cmdiad_auc_counts(const uint64_t* ok_sorted_keys, int n_ok, const double* def_score, int n_def, uint64_t* S,
                      cmdiad_stream_t stream);

/* hist [total_comp, T + 1] u32 (zeroed by the caller; at most 2^28 entries): hist[def_comp[i]][b] += 1 with b = the number of
 * thresholds strictly below def_score[i].  thr [T] f64 ascending, T <= 1024.  An id outside 0 .. total_comp - 1 is skipped. */
int cmdiad_pro_hist(const double* thr, int T, const double* def_score, const int32_t* def_comp, int n_def, int total_comp,
                    uint32_t* hist, cmdiad_stream_t stream);

/* ---- defect regions of score maps (docs/regions.md; additions, the ABI stays 6).  Everything but score_sum is an integer or a
 * stored double found by integer work (integer atomics only; no float goes through an atomic), so it is bit-exact whatever the
 * order of arrival.  Sizes as for the labelling: n in 0..65535, H, W >= 1, H * W <= 2^24, n * H * W <= 2^30; n == 0 returns
 * CMDIAD_OK without a launch. ---- */

/* mask [n,H,W] uint8 = maps [n,H,W] f64 > thr, a comparison of doubles (-0.0 > +0.0 is false; a NaN score is background).  thr lives
 * in DEVICE memory: [1] (thr_per_image = 0) or [n] (thr_per_image = 1), so a captured graph follows a threshold that is rewritten
 * between replays.  nan_count [1] int32 (NULL: not wanted) = NaN scores; zeroed first, also when n == 0. */
int cmdiad_threshold_mask(const double* maps, const double* thr, int thr_per_image, int n, int H, int W, uint8_t* mask,
                          int32_t* nan_count, cmdiad_stream_t stream);

/* The strongest regions of every image.  maps [n,H,W] f64 and the labels / n_comp / comp_offset / comp_size (comp_cap entries,
 * comp_cap >= n ceil(H/2) ceil(W/2)) of the labelling of their mask.  Among the components of image i with comp_size >= min_area,
 * count [n] int32 = how many there are, and the first max_regions (1..64) in the order (peak descending, label ascending; -0.0 and
 * +0.0 are one peak) go to slots 0 .. min(count, max_regions) - 1 of
 *   ints [n, max_regions, 8] int32: label, area, x0, y0, x1, y1 (inclusive box; x = column, y = row), peak_x, peak_y (the first
 *     pixel in raster order whose score equals the peak),
 *   vals [n, max_regions, 4] f64: peak (the stored double at peak_x, peak_y), score_sum, cx, cy (exact integer sums of the columns
 *     / rows, one f64 division by the area each).
 * The slots behind them are zero; count[i] > max_regions says the table was truncated.  score_sum is summed over the region's
 * bounding box in raster order with a fixed lane assignment and a fixed reduction tree: it depends on the component's pixels alone,
 * not on n, on i or on the run.  The per-component tables live in the workspace (8-byte aligned; the size query returns 0 for sizes
 * that are refused); every index into them is checked against n ceil(H/2) ceil(W/2).  The launch geometry depends on n, H, W only:
 * nothing is read back. */
size_t cmdiad_region_table_workspace_bytes(int n, int H, int W);
int cmdiad_region_table(const double* maps, const int32_t* labels, const int32_t* n_comp, const int32_t* comp_offset,
                        const int32_t* comp_size, int comp_cap, int n, int H, int W, int min_area, int max_regions, int32_t* count,
                        int32_t* ints, double* vals, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream);

/* The regions of a table in the units of the organised cloud (docs/regions.md, "Contract of a measurement table"; an addition, the
 * ABI stays 6).  labels [n,H,W], count [n] and ints [n,max_regions,8] as cmdiad_ccl_label / cmdiad_region_table leave them; cloud =
 * one float32 xyz per map pixel, coordinate c of pixel q of image i at cloud[i * 3 H W + q * pix_stride + c * ch_stride].  Only
 * planar [n,3,H,W] (pix_stride 1, ch_stride H W) and interleaved [n,H,W,3] (pix_stride 3, ch_stride 1) are accepted; both give
 * the same bits.  A point is valid iff its three coordinates are non-zero (-0.0 is zero) and finite.  For every slot
 * j < min(count[i], max_regions), over the pixels of its box that carry its label:
 *   m_ints [n, max_regions, 4] int32: n_pts (valid points), n_tri (triangles counted), peak_valid (the point at peak_x, peak_y is
 *     valid), 0;
 *   m_vals [n, max_regions, 20] f64: lo[3], hi[3] (per-axis minimum / maximum of the valid points, the stored floats widened),
 *     peak_xyz[3] (zeros unless peak_valid), s1[3] = sum (p - lo), s2[6] = sum (p - lo)_a (p - lo)_b for xx, xy, xz, yy, yz, zz,
 *     area = sum over the triangles (y,x), (y,x+1), (y+1,x+1) and (y,x), (y+1,x+1), (y+1,x) whose three vertices carry the label and
 *     are valid of 0.5 |(b - a) x (c - a)|, 0.  Every sum in float64 from the widened floats, no contraction.
 * A slot without a valid point and the slots behind min(count, max_regions) are zero.  One workgroup of 256 per (slot, image) walks
 * the box twice in the order of score_sum (thread t: positions t, t + 256, ...; the fixed butterfly; (w0 + w1) + (w2 + w3)): the
 * result does not depend on n, on i, on the layout or on the run, and no float goes through an atomic.  The table is not trusted:
 * count is clamped to [0, max_regions], boxes and peaks to the image, a label below 1 matches no pixel.  bad_count [1] int32 (NULL:
 * not wanted) = points of the whole frames with a non-finite coordinate; zeroed first, also when n == 0.  Sizes as for
 * cmdiad_region_table.  No allocation, no synchronisation, no workspace, no scratch. */
int cmdiad_region_measure(const int32_t* labels, const int32_t* count, const int32_t* ints, const float* cloud, long long pix_stride,
                          long long ch_stride, int n, int H, int W, int max_regions, int32_t* m_ints, double* m_vals,
                          int32_t* bad_count, cmdiad_stream_t stream);

/* ---- precision-recall numbers and defect detection counts (docs/metrics.md, "Precision-recall and detection counts"; additions,
 * the ABI stays 6).  Every result is an integer or a stored key picked by integer work (integer atomics only), so it is bit-exact
 * whatever the order of arrival; AP and the F1 value are float64 expressions of the caller over these integers.  Everywhere: every
 * argument is checked before any launch, a negative size or one above 2^30 is rejected, size 0 returns CMDIAD_OK without a launch,
 * nothing synchronises. ---- */

/* The run table of the defect scores.  def_sorted_keys [n_def] and ok_sorted_keys [n_ok]: the SORTED keys (cmdiad_f64_to_keys,
 * cmdiad_sort_u64) of the defect and of the defect-free scores.  A run is a maximal group of equal defect keys; runs are numbered in
 * ascending key order, r = 0 .. n_runs - 1, whatever the launch geometry:
 *   run_key [run_cap] u64 = the key, run_first [run_cap] int32 = the index of the run's first element in def_sorted_keys,
 *   run_fp [run_cap] int32 = n_ok - #(ok keys < key) = the defect-free scores at or above the run's value; n_runs [1] int32.
 * tp = n_def - run_first defect scores lie at or above the run's value; the run holds run_first[r + 1] - run_first[r] of them.
 * Nothing is written past run_cap entries (n_runs still has the true number; run_cap = n_def always suffices).  n_def == 0 zeroes
 * n_runs (where it is passed) and launches nothing.  The tile query returns the keys per block of the head count and compaction
 * passes: sizes around its multiples are where the passes change shape.  The scratch is a typed buffer of the caller's, like the
 * outputs, and its size is a formula, so there is no size query: tile_heads [tile_cap] int32 with tile_cap >= 2 ceil(n_def / tile)
 * holds the run heads per tile and behind them their exclusive scan; both are left there. */
size_t cmdiad_pr_tile(void);
int cmdiad_pr_runs(const uint64_t* def_sorted_keys, int n_def, const uint64_t* ok_sorted_keys, int n_ok, uint64_t* run_key,
                   int32_t* run_first, int32_t* run_fp, int run_cap, int32_t* n_runs, int32_t* tile_heads, int tile_cap,
                   cmdiad_stream_t stream);

/* best [2] int64 = (the run r that maximises F1[r] = 2 tp / (tp + fp + n_def) with tp = n_def - run_first[r], fp = run_fp[r]; 0,
 * reserved).  Fractions are compared exactly, by cross-multiplication in unsigned 64-bit; among equal fractions the largest r (the
 * highest threshold) wins: a total order, so the answer does not depend on the reduction tree.  n_runs [1] int32 is read on the
 * DEVICE and clamped to 0..run_cap; a run with run_first outside 0..n_def - 1 or a negative run_fp is passed over; best[0] = -1 when
 * no run is left.  The table is plain integers: it need not come from cmdiad_pr_runs.  Two launches: the first stage's block b takes
 * the runs [256 j, 256 j + 256) for j = b, b + blocks, ... with blocks = min(ceil(run_cap / 256), 1024).  partial
 * [partial_cap] int32, partial_cap >= blocks (1024 always suffices): the first stage's winners, a typed scratch buffer of the
 * caller's.  run_cap == 0 launches nothing and leaves best alone. */
int cmdiad_pr_f1max(const int32_t* run_first, const int32_t* run_fp, const int32_t* n_runs, int run_cap, int n_def, int64_t* best,
                    int32_t* partial, int partial_cap, cmdiad_stream_t stream);

/* Overlap of two labellings of the same n frames [n,H,W] (both as cmdiad_ccl_label leaves them): the ground truth's (gt_labels,
 * gt_comp_offset [n + 1]) and the prediction's (pred_labels, pred_comp_offset [n + 1], pred_comp_size [pred_comp_cap]).  A predicted
 * component is KEPT when its size is at least min_area (>= 1).  covered [gt_comp_cap] int32: per ground-truth component (global id)
 * its pixels that lie in a kept predicted component; hits [pred_comp_cap] int32: per predicted component the ground-truth pixels
 * inside it, 0 for one that is not kept.  Both are zeroed first.  Every id is checked against the capacity of the table it indexes;
 * sizes as for the labelling. */
int cmdiad_region_overlap(const int32_t* gt_labels, const int32_t* gt_comp_offset, int gt_comp_cap, const int32_t* pred_labels,
                          const int32_t* pred_comp_offset, const int32_t* pred_comp_size, int pred_comp_cap, int n, int H, int W,
                          int min_area, int32_t* covered, int32_t* hits, cmdiad_stream_t stream);

/* counts [n,4] int32 per image: n_gt (its ground-truth components), n_detected (those with covered > 0), n_pred (its kept predicted
 * components), n_false (kept ones with hits == 0), from the tables of cmdiad_region_overlap.  Offsets are clamped to the capacities:
 * nothing is read outside them. */
int cmdiad_detection_counts(const int32_t* gt_comp_offset, const int32_t* covered, int gt_comp_cap, const int32_t* pred_comp_offset,
                            const int32_t* pred_comp_size, const int32_t* hits, int pred_comp_cap, int n, int min_area,
                            int32_t* counts, cmdiad_stream_t stream);

/* ---- xyz TIFFs (docs/tiff.md; utils/mvtec3d_util.py:9-11 of the reference reads them with tifffile on the host) ----
 * raw [raw_bytes] = file bytes with UNCOMPRESSED chunks (dword aligned, raw_bytes a multiple of 4: the upload buffer is padded),
 * chunk_off [B, n_chunks] (device) = byte offset into raw of every chunk of every image -> out [B,H,W,C] of the files' own float type
 * (bytes_per_sample 4 | 8), in the device's byte order.  A strip is a tile of full width (chunk_w == W, chunk_h = rows per strip);
 * chunks are numbered row-major over the image, plane after plane when planar (n_chunks must equal what the geometry gives).
 * predictor 1: a copy with a byte swap when big_endian; predictor 3: libtiff's floating-point predictor is undone per chunk row
 * (chunk_w * (planar ? 1 : C) * bytes_per_sample bytes, at most 64 KiB), big_endian is then not looked at.  Offsets need no
 * alignment.  Any source byte outside [0, raw_bytes) reads as 0: no table makes the kernels read outside raw.  Tile padding and the
 * missing rows of a short last strip are neither read as samples nor written.  B in 1..65535, sides in 1..16384, C in 1..4. */
int cmdiad_tiff_unpack(const uint8_t* raw, int64_t raw_bytes, const int64_t* chunk_off, int B, int n_chunks, int W, int H, int C,
                       int chunk_w, int chunk_h, int planar, int bytes_per_sample, int big_endian, int predictor, void* out,
                       cmdiad_stream_t stream);

/* ---- the datasets' PNGs (docs/png.md; the reference decodes them with Pillow on the host, dataset.py:103, 225, 239) ----
 * raw [raw_bytes] holds, at offsets[b] (device, [B]) for every image b, its INFLATED and still FILTERED scanlines: H rows of
 * 1 + W * bpp bytes, the filter type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; anything above acts as None) in front of each row;
 * bpp = bytes per pixel = channels of an 8-bit file (1 grey, 2 grey + alpha, 3 rgb, 4 rgb + alpha).  The filters are undone and the
 * pixels stored converted -> out uint8: target 0 'rgb' [B,H,W,3] (alpha dropped, grey replicated), 1 'l' [B,H,W] (the grey byte, or
 * (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16), 2 'raw' [B,H,W,bpp] (the file's own channels).  One workgroup per image;
 * waves = 0 lets the width choose its waves (8 up to 897 pixels, 16 up to 1857, else 1), 1 | 8 | 16 force them (8 and 16 within
 * those widths only).  Offsets need no alignment.  Any source byte outside [0, raw_bytes) reads as 0: no offset makes the kernel
 * read outside raw.  No allocation, no synchronisation, no scratch.  B in 1..65535, sides in 1..16384 (a row is at most 64 KiB). */
int cmdiad_png_unfilter(const uint8_t* raw, int64_t raw_bytes, const int64_t* offsets, int B, int W, int H, int bpp, int target,
                        int waves, uint8_t* out, cmdiad_stream_t stream);

/* The encoder's side (utils/png.py: encode, write_many; an addition, the ABI stays 6): images [n,H,W,C] uint8, C in 1..4 ->
 * scanlines [n, H * (1 + W * C)], every row its filter byte and then its filtered bytes -- the layout above.  mode 0..4 forces that
 * filter type on every row; mode 5 is adaptive: per row the type with the smallest sum of m(b) = b < 128 ? b : 256 - b over its
 * filtered bytes, ties to the lowest type.  Row 0 sees a zero prior row, bytes before the first pixel see zero, Paeth is the
 * standard predictor.  One wave per row, integer wave reductions: the result does not depend on any order.  n in 0..65535 (0 returns
 * CMDIAD_OK without a launch), sides in 1..16384.  No allocation, no synchronisation, no scratch. */
int cmdiad_png_filter(const uint8_t* images, int n, int H, int W, int C, int mode, uint8_t* scanlines, cmdiad_stream_t stream);

/* ---- anomaly overlays (docs/overlay.md; an addition, the ABI stays 6) ----
 * maps [n,H,W] f64 -> canvas [n,Ho,Wo,3] uint8 in one launch.  Per canvas pixel (x, y), every floating-point step one float64
 * operation, rounded once, in this order:
 *   score  u = (x + 0.5) * (W / Wo) - 0.5 clamped to [0, W - 1], x0 = floor(u), x1 = min(x0 + 1, W - 1), fx = u - x0, the same for y;
 *          s = (m[y0,x0] (1 - fx) + m[y0,x1] fx) (1 - fy) + (m[y1,x0] (1 - fx) + m[y1,x1] fx) fy, where a tap (or row) whose weight is
 *          exactly 0 is neither read nor added: Ho == H and Wo == W reproduce the map bit for bit, infinities included.
 *   index  d = hi - lo; t = d > 0 ? (s - lo) / d : (s > lo ? 1 : 0), clamped to [0, 1] (a NaN t is 0); a NaN s gives t = 0 and is
 *          counted; k = (int)floor(t * 255 + 0.5).  lohi lives in DEVICE memory: [2] (lohi_per_image = 0) or [n,2] (1).
 *   colour c = lut[k] (lut [256,3] uint8, device), a = alpha[k] (alpha [256] uint8, device); per channel
 *          out = (c a + bg (255 - a) + 127) / 255 in integers.  bg_kind 0: no background, out = c; 1: bg uint8 [n,Ho,Wo,3];
 *          2: bg float32 [n,3,Ho,Wo], byte = clamp(floor((v std + mean) 255 + 0.5), 0, 255) in float64 from the widened float.
 *   contour (thr != NULL; thr in DEVICE memory, [1] or [n] by thr_per_image, as cmdiad_threshold_mask) the pixel takes contour_rgb iff
 *          s > thr and one of its four neighbours inside the canvas has !(s > thr); strict, a NaN is never above.
 *   boxes  (count [n] and ints [n,K,8] of cmdiad_region_table, both or neither) slot j < min(count, K) with the map box x0, y0, x1, y1:
 *          X0 = x0 Wo / W, X1 = ((x1 + 1) Wo + W - 1) / W - 1 (integer division; Y alike), clamped to the canvas; the pixel takes
 *          box_rgb iff it lies in the box and fewer than line_px (1..8) pixels from its border.  Boxes go over contours.
 * Colours are r | g << 8 | b << 16.  nan_count [1] int32 (NULL: not wanted) = canvas pixels with a NaN score; zeroed first, also when
 * n == 0.  n in 0..65535, sides in 1..16384, n H W and n Ho Wo <= 2^30, K in 1..64 (checked also without tables).  Ho Wo a multiple
 * of 4 with a 4-byte aligned canvas (and background: 4 bytes for kind 1, 16 for kind 2) takes dword stores; anything else byte
 * stores, with the same result.  No allocation, no synchronisation, no scratch. */
int cmdiad_overlay_render(const double* maps, int n, int H, int W, int Ho, int Wo, const double* lohi, int lohi_per_image,
                          const double* thr, int thr_per_image, const void* bg, int bg_kind, double mean_r, double mean_g, double mean_b,
                          double std_r, double std_g, double std_b, const uint8_t* lut, const uint8_t* alpha, const int32_t* count,
                          const int32_t* ints, int K, int line_px, uint32_t contour_rgb, uint32_t box_rgb, uint8_t* canvas,
                          int32_t* nan_count, cmdiad_stream_t stream);

/* ---- scored scans as coloured PLY meshes (docs/mesh.md; an addition, the ABI stays 6) ----
 * cloud as for cmdiad_region_measure (one float32 xyz per map pixel, the two element strides, planar or interleaved: the same
 * bytes), maps [n,H,W] f64 at the cloud's H, W.  A point is valid iff its three coordinates are non-zero (-0.0 is zero) and finite.
 *   vertices  the valid pixels of an image in raster order; vidx [n,H,W] int32 = each pixel's rank, -1 for an invalid pixel.
 *   faces     cell (y, x), y + 1 < H and x + 1 < W: T0 = (y,x), (y,x+1), (y+1,x+1) and T1 = (y,x), (y+1,x+1), (y+1,x); a triangle is
 *             emitted iff its three vertices are valid and each edge has d2 = (dx dx + dy dy) + dz dz <= max_edge2, the differences
 *             in float64 from the widened floats, every step one float64 operation.  Cells in raster order, T0 before T1; flip = 1
 *             stores a, c, b.  max_edge2 = +inf cuts nothing; a NaN or a value <= 0 is refused.
 *   normal    of vertex (y, x): the sum from 0.0, per component, of (b - a) x (c - a) -- each component two products and one
 *             difference, the triangle's own a, b, c -- over the emitted ones of cell (y-1,x-1) T0, T1, cell (y-1,x) T1, cell (y,x-1)
 *             T0, cell (y,x) T0, T1, in this order; len = sqrt((nx nx + ny ny) + nz nz); (float)(n / len) when len > 0 and finite,
 *             else zeros; flip = 1 negates the three floats.
 *   colour    cmdiad_overlay_render's index and colour steps on s = maps[i,y,x]; bg at the maps' size (kind 0 | 1 | 2).
 *   records   vertex, 35 bytes little-endian: float x y z (the stored bits), float nx ny nz, uchar red green blue, float score (the
 *             float64 rounded once), int region (labels [n,H,W] int32, or 0 when labels is NULL).  Face, 13 bytes: uchar 3 and three
 *             int32 vertex ranks.  Image i fills the front of its slot densely: vertices + i H W 35, faces + i 2 (H-1) (W-1) 13.
 * cmdiad_mesh_count (one memset, one kernel): chunks [n, C, 2] int32, C = ceil(H W / 1024) = vertices and faces of every run of 1024
 * pixels; counts [n,4] int32 = n_vert, n_face, bad (points with a non-finite coordinate), nan (valid vertices with a NaN score;
 * they take t = 0).  cmdiad_mesh_write (two kernels; one where H or W is 1, and faces may then be NULL) takes that chunks table and
 * writes vidx and the two record buffers; a table that does not belong to the cloud cannot make it write outside a slot.  Integer
 * atomics only: the result does not depend on n, on i, on the layout or on the run.  n in 0..65535 (0 returns CMDIAD_OK without a
 * launch), sides in 1..16384, n H W <= 2^24.  No workspace, no allocation, no synchronisation, no scratch. */
int cmdiad_mesh_count(const float* cloud, long long pix_stride, long long ch_stride, const double* maps, int n, int H, int W,
                      double max_edge2, int32_t* chunks, int32_t* counts, cmdiad_stream_t stream);
int cmdiad_mesh_write(const float* cloud, long long pix_stride, long long ch_stride, const double* maps, int n, int H, int W,
                      const double* lohi, int lohi_per_image, const uint8_t* lut, const uint8_t* alpha, const void* bg, int bg_kind,
                      double mean_r, double mean_g, double mean_b, double std_r, double std_g, double std_b, const int32_t* labels,
                      double max_edge2, int flip, const int32_t* chunks, int32_t* vidx, uint8_t* vertices, uint8_t* faces,
                      cmdiad_stream_t stream);

/* ---- unordered point clouds into the pixel grid (docs/organize.md; an addition, the ABI stays 6) ----
 * points [P,3] float32: the clouds of a batch back to back; offsets [n+1] int64 ON THE DEVICE, not trusted: cloud b is the points
 * [lo_b, hi_b), lo_b = clamp(offsets[b], 0, P), hi_b = clamp(offsets[b+1], lo_b, P), and only its first max_len points are looked
 * at (max_len sizes the launch: pass the longest cloud).  cams [n,16] f64: a row-major 3 x 4 transform T, then a, b, c, d.
 *   c_k = ((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3], k = 0, 1, 2, on the widened floats
 *   kind 0 (orthographic, a b c d = x0 y0 sx sy): u = (c0 - x0) sx, v = (c1 - y0) sy
 *   kind 1 (pinhole, a b c d = fx fy cx cy):      u = fx (c0 / c2) + cx, v = fy (c1 / c2) + cy, and c2 > 0 is required
 *   uf = floor(u + 0.5), vf = floor(v + 0.5); inside iff 0 <= uf < W and 0 <= vf < H, compared as doubles (a NaN is outside), and
 *   d32 = (float)c2 with -0.0 taken as +0.0 is finite.  Every step is one float64 operation, in this order.
 * A point with a non-finite or a zero coordinate is dropped (the package's rule for an invalid pixel), any other point that is not
 * inside is outside, the rest are placed: key = ord(d32) << 32 | (i - lo_b), ord the map under which unsigned order is float order
 * (sign bit set: all bits inverted; else the sign bit set), and the pixel keeps the smallest key: the nearest d32, the lowest index
 * among equal ones.
 * cmdiad_cloud_bounds (three kernels): bounds [n,6] f64 = the minimum of c_0, c_1, c_2, then the maximum, over the cloud's valid (not
 * dropped) points; count [n] int32 = their number.  A NaN c_k enters neither, a zero of either sign counts as +0.0, an empty cloud
 * gives +inf, -inf and 0.  Between its kernels bounds holds 64-bit ordered keys: no other scratch.
 * cmdiad_organize_splat (two kernels): keys [n,H,W] uint64 = all ones, then the minimum over the placed points; pixel_of_point [P]
 * int32 = -2 dropped, -1 outside, vf W + uf placed, written for the points looked at only; stats [n,4] int32 columns 0 and 1 =
 * dropped, outside (zeroed here; columns 2 and 3 are left alone).
 * cmdiad_organize_resolve (two kernels): a pixel whose key is not all ones is a direct hit; any other takes, with fill = r in 1..2,
 * the smallest key of the (2r+1)^2 window clipped to the image (direct hits only: fills do not cascade) and is then filled.  A key
 * whose index is not below hi_b - lo_b is an empty pixel.  index [n,H,W] int32 = the winner's index in its cloud or -1; xyz [n,H,W,3]
 * float32 = its three input floats, bit for bit, or zeros; rgb [n,H,W,3] uint8 (NULL: not wanted) = colors [P,3] uint8 of the winner
 * (NULL: 0), or 0; mask [n,H,W] uint8 (NULL: not wanted) = 255 where labels [P] uint8 of the winner is not 0 (NULL: 0); stats
 * columns 2 and 3 = direct, filled pixels (zeroed here; columns 0 and 1 are left alone).
 * Integer atomics only (a 64-bit minimum, one 32-bit add per workgroup): the result does not depend on the run.  n in 0..65535 (0
 * returns CMDIAD_OK without a launch), H W <= 2^24, n H W <= 2^30, P and max_len in 0..2^31-1.  No workspace, no allocation, no
 * synchronisation, no scratch. */
int cmdiad_cloud_bounds(const float* points, const int64_t* offsets, const double* cams, int n, int P, int max_len, double* bounds,
                        int32_t* count, cmdiad_stream_t stream);
int cmdiad_organize_splat(const float* points, const int64_t* offsets, const double* cams, int n, int P, int max_len, int kind, int H,
                          int W, uint64_t* keys, int32_t* pixel_of_point, int32_t* stats, cmdiad_stream_t stream);
int cmdiad_organize_resolve(const float* points, const int64_t* offsets, const uint8_t* colors, const uint8_t* labels,
                            const uint64_t* keys, int n, int P, int H, int W, int fill, int32_t* index, float* xyz, uint8_t* rgb,
                            uint8_t* mask, int32_t* stats, cmdiad_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Content digest (stored fits: cmdiad_amd/fitted.py, docs/fitted.md)
 * ------------------------------------------------------------------------------------------- */

/* 64-bit digest of a device buffer, ADDED into *acc (one device uint64 that the caller zeroes; several calls may add into the same
 * one).  With w_i the n = bytes / 4 little-endian 32-bit words of the buffer and h the splitmix64 finaliser
 *   h(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31      (mod 2^64)
 *   digest(buf, seed) = sum_i h( h(seed + i) ^ w_i )   mod 2^64.
 * The sum is commutative and associative mod 2^64: any reduction order gives the same bits (one 64-bit atomic add per workgroup,
 * nothing else), and digest(a || b, s) = digest(a, s) + digest(b, s + len(a) / 4), so a buffer can be hashed in pieces.
 * The digest guards against MISTAKES -- a fit loaded next to another checkpoint, a truncated or damaged file, a wrong row shard --
 * NOT against adversaries: collisions are easy to construct on purpose.
 * data needs 4-byte alignment only (16-byte loads with a head and a tail path).  bytes % 4 != 0, a data pointer that is null
 * (with bytes > 0) or not 4-byte aligned, or a null acc return CMDIAD_ERR_ARG and touch nothing; bytes == 0 is a success that
 * leaves *acc unchanged.  No workspace, no allocation, no synchronisation.  (New with ABI 6; the version is unchanged, as for
 * earlier added entry points.) */
int cmdiad_digest64(const void* data, size_t bytes, uint64_t seed, uint64_t* acc, cmdiad_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CMDIAD_HIP_H */
