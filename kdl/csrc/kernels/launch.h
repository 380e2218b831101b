// Host-side launch API of the kdl HIP kernel library. Every launcher is
// asynchronous on the given stream, allocates nothing and synchronises nothing,
// so any sequence of them can be captured into a hipGraph (cdna guide G9).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kdl {

struct ConvGemmArgs {
  const uint16_t* x;     // input activations NHWC bf16, channel stride ldx
  const uint16_t* wp;    // packed weights [NF][K/32][64][8] bf16 (BN scale folded)
  const float* bias;     // [NF*16] fp32 (BN shift)
  const float* dww;      // MODE_DW: depthwise weights [9][K] fp32
  const uint16_t* dwk;   // MODE_DW, sepconv_ws / sepconv_2d: the same weights as bf16 entries [K/32][2][16][2][8]
                         //   (k-step, channel group, channel, tap parity, taps parity+2j)
  const uint16_t* res;   // optional residual [M][ldr] bf16
  uint16_t* y;           // output [M][ldy] bf16 (or a zero-bordered [B][OH+2][OW+2][ldy] if opad)
  int B, H, W;           // input spatial dims
  int OH, OW;            // output spatial dims
  int M;                 // B*OH*OW
  int ldx, ldy, ldr;     // channel strides (elements)
  int K;                 // reduction depth (multiple of 32)
  int cin;               // MODE_CONV: padded input channels (multiple of 32)
  int NF;                // 16-wide output-channel fragments in the packed weights
  int nstore;            // output channels written (<= ldy)
  int stride;            // spatial stride (MODE_PW / MODE_CONV)
  int relu_in;
  int relu_out;          // 0 none; 1 ReLU before the residual add (Xception); 2 after it (ResNet);
                         // 3 exact GELU before the residual add (ViT MLP); 4 SiLU before it (EfficientNet)
  unsigned long long* stamps;  // diagnostics only (stamping kernel variants): per-wave s_memtime per k-step
  int opad;              // 1: write into the interior of a 1-pixel zero-bordered output buffer, so the
                         //    next 3x3 'same' conv runs as a 'valid' implicit GEMM with no bounds checks;
                         // 2: token rows behind a class token: row m -> b*(OH*OW+1) + 1 + m%(OH*OW)
  int dt;                // element type of x / wp / res / y: 0 bf16, 1 fp16 (MODE_PW / MODE_CONV GEMMs)
  // LDS-DMA pipelined GEMM (gemm_pipe): 1 = every M tile walks K from its own starting
  // step ((7*mi) mod K/32), so the workgroups sharing the weights do not all fetch the same
  // fragments at launch (env KDL_PIPE_KROT overrides; 0 = in order)
  int krot;
  // split-K (gemm_pipe only; ResNet-50's layer3/4 3x3 convs: M = 6272 / 1568 rows fill a quarter to a
  // half of the 256 CUs with whole-K tiles): ksplit > 1 workgroups per output tile each reduce K/ksplit
  // k-steps into fp32 partials at ws ([ksplit][tiles][BM*BN], fragment-linear); the last of a tile to
  // arrive (per-tile counter cnt, agent-scope release/acquire, reset to 0 by that workgroup) sums
  // them and runs the normal epilogue. K/32 must divide by ksplit.
  int ksplit;
  float* ws;
  int* cnt;
  // per-image channel scales on the A operand (EfficientNet project conv: the SE scale, gemm_pipe
  // MODE_PW bf16 only): A[m][k] is multiplied by ascale[image(m) * ascale_ld + k] on its way from
  // LDS to the MFMA (round 6; it replaced per-image SE-scaled weight copies); M tiles then never
  // straddle two images. nullptr = no scale.
  const float* ascale;
  int ascale_ld;
};

// cfg < PIPE_CFG_BASE: register-B kernel (all modes, incl. fused depthwise);
// cfg >= PIPE_CFG_BASE: LDS-DMA pipelined kernel (MODE_PW / MODE_CONV only).
constexpr int PIPE_CFG_BASE = 16;
// cfg >= SEP_CFG_BASE: fused separable convs (MODE_DW only). Ids 64..119 are retired (the
// round-1/2 sepconv_fused / sepconv_pipe kernels, measured slower than sepconv_ws / sepconv_2d
// on every Xception shape and removed in round 3).
constexpr int SEP_CFG_BASE = 64;
// cfg >= SEPW_CFG_BASE: warp-specialized fused separable conv (sepconv_ws.hip).
constexpr int SEPW_CFG_BASE = 120;
hipError_t sepconv_ws(int cfg, const ConvGemmArgs& a, hipStream_t s);
int sepconv_ws_config(int cfg, int* bm, int* bn, int* threads);
int sepconv_ws_fits(int cfg, int W);

// A whole Xception entry block (SeparableConv -> ReLU -> SeparableConv -> 3x3/2 max-pool, plus
// the 1x1/2 residual conv) in one persistent launch, entry_block.hip. Workgroup g runs the
// host-built steps [step_off[g], step_off[g+1]) of `steps`: int4 {image, strip, pooled row k,
// mode} with mode 0 = warm-up (y1 only), 1 = warm-up (y1 + y2, no output), 2 = output row k.
struct EntryBlockArgs {
  const uint16_t* x;      // block input [B][H][W][ldx] bf16
  uint16_t* y;            // block output [B][OH][OW][ldy] bf16
  const uint16_t* w1;     // sepconv1 pointwise, packed [C1/16][C0/32][64][8] (BN scale folded)
  const float* b1;        // [C1] BN shift
  const float* dw1;       // sepconv1 depthwise [9][C0] fp32
  const uint16_t* w2;     // sepconv2 pointwise, packed [C1/16][C1/32][64][8]
  const float* b2;
  const float* dw2;       // [9][C1]
  const uint16_t* dwk1;   // the same depthwise weights as pack_dw_entries (MFMA depthwise configs)
  const uint16_t* dwk2;
  const uint16_t* wr;     // residual 1x1/2 conv, packed [C1/16][C0/32][64][8]
  const float* br;
  int B, H, W, OH, OW, ldx, ldy;
  int grid;               // workgroups (= len(step_off) - 1)
  const int4* steps;
  const int* step_off;
  unsigned long long* stamps;   // stamping configs (id >= 100) only: [8 wg][64 steps][5 phases]
};
hipError_t entry_block(int cfg, const EntryBlockArgs& a, hipStream_t s);
int entry_block_config(int cfg, int* c0, int* c1, int* pc, int* lds);

// cfg >= C3_CFG_BASE: 3x3 'valid' conv over 2-D tiles with an LDS halo patch (MODE_CONV, cin 32 only,
// conv3x3_2d.hip: Xception block1_conv2).
constexpr int C3_CFG_BASE = 208;
hipError_t conv3x3_2d(int cfg, const ConvGemmArgs& a, hipStream_t s);
int conv3x3_2d_config(int cfg, int* bm, int* bn, int* threads);
// cfg >= S2D_CFG_BASE: fused separable conv over 2-D spatial tiles (MODE_DW only, sepconv_2d.hip).
constexpr int S2D_CFG_BASE = 160;
hipError_t sepconv_2d(int cfg, const ConvGemmArgs& a, hipStream_t s);
int sepconv_2d_config(int cfg, int* bm, int* bn, int* threads);
// cfg == STREAM_CFG_BASE (+1: nontemporal output stores): persistent streaming pointwise GEMM, weights
// resident in LDS (MODE_PW, stride 1, small K; the (K, N) shapes of gemm_stream.hip's instance list
// only; per-image weights ok).
constexpr int STREAM_CFG_BASE = 3000;
hipError_t gemm_stream(const ConvGemmArgs& a, bool nt, hipStream_t s);
bool gemm_stream_shape(int K, int nstore, int dt = 0);
hipError_t conv_gemm(int mode, int cfg, const ConvGemmArgs& a, hipStream_t s);
hipError_t gemm_pipe(int mode, int cfg, const ConvGemmArgs& a, hipStream_t s);
int gemm_pipe_config(int cfg, int* bm, int* bn, int* threads);
int conv_gemm_config(int cfg, int* bm, int* bn, int* threads);
int conv_gemm_num_configs();

// Depthwise 3x3 'same' (+ReLU on load): NHWC bf16 [B][H][W][C] -> same layout.
struct DwArgs {
  const uint16_t* x;
  const float* w;         // [9][C] fp32
  uint16_t* y;
  int B, H, W, C;         // C = padded channel stride (multiple of 8)
  int relu_in;
  int cg, rb, tw, seg;    // tile overrides (0 = host heuristic): 8-ch chunks, rows, cols, cols/item
  int algo;               // 0 = auto, 1 = LDS-tiled, 2 = direct row-streaming (rb / seg / pd apply)
  int pd;                 // direct kernel: input rows prefetched ahead (0 = default)
};
hipError_t dw3x3(const DwArgs& a, hipStream_t s);

// Stem: 3x3 stride-2 'valid' conv, 3 input channels -> 32, + bias + ReLU.
// in_kind: 0 = uint8 HWC pixels (Xception normalisation folded into weights),
//          1 = fp32 HWC already preprocessed (TF-Serving compat input).
struct StemArgs {
  const void* x;
  const uint16_t* wp;     // packed [cout/16][K32][64][8], k = (ky*KW+kx)*3 + c
  const float* bias;      // [cout]
  uint16_t* y;            // [B*OH*OW][ldy]
  int B, H, W, OH, OW, ldy;       // OH, OW at most (H + 2 pad - K) / stride + 1; ldy multiple of 8
  int in_kind;
  int KH, KW, stride, pad, cout;  // generic KxK stride/pad conv from 3 channels (cout = 32 or 64)
  float scale[3], shift[3];       // per-channel input normalisation applied on load (zero padding
                                  // stays exact: padded taps are 0 in the normalised space)
  int relu;                       // 0 none, 1 ReLU, 2 SiLU
  int dt;                         // output element type: 0 bf16, 1 fp16
  int rows;                       // 1: row-run K layout (k = ky*RP + kx*3 + c, RP = 32 for 7x7,
                                  // 16 for 3x3; stem_rows_kernel); 0: k = (ky*KW+kx)*3 + c
};
hipError_t stem_conv(const StemArgs& a, hipStream_t s);

// Xception block1_conv1 + block1_conv2 in one launch (stem_conv3x3.hip): the 3x3/2 'valid' stem
// (uint8 image, 3 -> 32, bias + ReLU; normalisation folded into the weights) is computed per tile
// of the following 3x3 'valid' stride-1 conv (32 -> NF*16, bias, optional ReLU); the 32-channel
// map in between lives only in LDS. Same values as stem_conv (rows = 1) followed by conv3x3_2d.
struct StemConvArgs {
  const uint8_t* x;       // [B][H][W][3] uint8
  const uint16_t* wp1;    // stem weights, packed [2][2][64][8], row-run K layout (k = ky*16 + kx*3 + c)
  const float* b1;        // [32]
  const uint16_t* wp2;    // second conv, packed [NF][9][64][8] (k = tap*32 + c)
  const float* b2;        // [NF*16]
  uint16_t* y;            // [B][OH][OW][ldy] bf16
  int B, H, W;            // image
  int H1, W1;             // stem map: (H-3)/2+1, (W-3)/2+1
  int OH, OW;             // output: H1-2, W1-2
  int ldy, NF, nstore;    // output channel stride; 16-wide fragments in wp2; channels written
  int relu_out;           // 0 none, 1 ReLU
  int grid;               // cap on the workgroups (0 = every resident workgroup of the chip)
};
// cfg: KDL_SC3_CONFIGS (tile of conv3x3_2d's config 7; producer waves / ring depth)
hipError_t stem_conv3x3(int cfg, const StemConvArgs& a, hipStream_t s);
int stem_conv3x3_config(int cfg, int* bm, int* bn, int* threads);

// TF-'same' 3x3/2 max-pool of `x` plus `res` (Xception entry/exit block tail).
struct PoolAddArgs {
  const uint16_t* x;      // [B][H][W][C]
  const uint16_t* res;    // [B][OH][OW][C] or null
  uint16_t* y;            // [B][OH][OW][C]
  int B, H, W, OH, OW, C; // C multiple of 8
  int pad_top, pad_left;
  int dt;                 // element type: 0 bf16, 1 fp16
  int algo;               // 0 auto, 1 pixel-per-thread, 2 row-streaming (seg / rb apply)
  int seg, rb;            // row-streaming: output columns per thread, output rows per band (0 = plan)
};
hipError_t pool_add(const PoolAddArgs& a, hipStream_t s);

// Global average pool: x [B][HW][ldx] bf16 -> y [B][F] fp32.
struct GapArgs {
  const uint16_t* x;
  float* y;               // [B][F] fp32 (may be null)
  uint16_t* yb;           // [B][F] bf16 copy for the MFMA classifier (may be null)
  int B, HW, ldx, F;      // F multiple of 8
  int dt;                 // element type of x and yb: 0 bf16, 1 fp16
};
hipError_t gap(const GapArgs& a, hipStream_t s);

// Dense layer on pooled features: out[b][n] = sum_k x[b][k] w[k][n] + bias[n] (+ReLU), fp32.
struct FcArgs {
  const float* x;         // [B][F]
  const float* w;         // [F][N] (Keras Dense / transposed torch Linear layout)
  const float* bias;      // [N]
  float* out;             // [B][N]
  int B, F, N, relu;
};
hipError_t fc(const FcArgs& a, hipStream_t s);

// MFMA classifier: out[b][n] = sum_k xb[b][k] W[n][k] + bias[n] (+ReLU), fp32 out.
// xb: bf16 [rows >= round_up(B,16)][F] (rows >= B zero), wp: packed [NF][F/32][64][8].
struct FcMfmaArgs {
  const uint16_t* xb;
  const uint16_t* wp;
  const float* bias;
  float* out;
  int B, F, N, NF, relu;
  int dt;                 // element type of xb and wp: 0 bf16, 1 fp16
};
hipError_t fc_mfma(const FcMfmaArgs& a, hipStream_t s);

// ViT patch embedding input: uint8 NHWC image -> A [B*np][3*P*P] bf16, k = c*P*P + ky*P + kx,
// normalised on load (per-channel scale/shift).
struct PatchifyArgs {
  const uint8_t* x;
  uint16_t* y;
  int B, H, W, P, ldy;
  float scale[3], shift[3];
};
hipError_t patchify(const PatchifyArgs& a, hipStream_t s);

// Token finalise: x [B][T][D] bf16 (rows 1..T-1 = patch embeddings); row 0 := cls + pos[0],
// rows t >= 1 += pos[t]. cls [D], pos [T][D] fp32.
struct EmbedArgs {
  uint16_t* x;
  const float* cls;
  const float* pos;
  int B, T, D;
};
hipError_t embed_tokens(const EmbedArgs& a, hipStream_t s);

// LayerNorm over the last dim (D <= 2048): y[r][:D] = LN(x[r*ldx .. +D]) * gamma + beta, bf16.
struct LnArgs {
  const uint16_t* x;
  uint16_t* y;
  uint8_t* y8;            // optional e4m3 output (value * inv_scale) instead of y
  float inv_scale;
  const float* gamma;
  const float* beta;
  long rows;
  int D, ldx, ldy;
  float eps;
};
hipError_t layernorm(const LnArgs& a, hipStream_t s);

// Multi-head self-attention (flash-style, online softmax) over a packed QKV buffer:
// qkv [B*T][3*H*dh] bf16 (q | k | v, head-major inside each), out [B*T][H*dh] bf16.
// Two kernels compute the same values: the whole-head one (one workgroup per (image, head),
// all keys in LDS, T <= 256) and the query-tiled one (64 queries per workgroup, any T).
// dh != 64, T <= 0, H <= 0, B <= 0, an algo outside 0..2 and algo 1 with T > 256 are
// hipErrorInvalidValue, and nothing is launched.
struct AttnArgs {
  const uint16_t* qkv;
  uint16_t* out;
  uint8_t* out8;          // optional e4m3 output (value * inv_scale) instead of out
  float inv_scale;
  int B, T, H, dh;        // dh = 64
  float scale;            // 1/sqrt(dh)
  int algo;               // 0 = auto (whole-head if T <= 256, unless env KDL_ATTN_TILED forces the
                          // query-tiled kernel), 1 = whole-head, 2 = query-tiled
};
hipError_t attention(const AttnArgs& a, hipStream_t s);

// MBConv depthwise KxK (K 3/5, stride S 1/2, symmetric pad) + bias (+SiLU) with the SE
// average pool and squeeze FC fused: pool[b][part][Cs] = sum over the part's channels of
// w1[j][c] * (sum of the part's outputs of channel c); part = (band, column tile, group).
struct DwkArgs {
  const uint16_t* x;      // [B][H][W][C]
  const float* w;         // [K*K][C] fp32 (BN scale folded)
  const float* bias;      // [C]
  uint16_t* y;            // [B][OH][OW][C]
  float* pool;            // null: no SE
  const float* w1;        // SE fc1 [Cs][C]
  int B, H, W, C, OH, OW, K, S, pad, act;   // act: 0 none, 2 SiLU
  int Cs;
  int cg, rb, tw, seg;    // tile override (0: host heuristic; tools/dwkbench.py sweeps these)
  int lds_kb;             // heuristic's LDS budget per workgroup (0: default)
  int algo;               // 0 auto, 1 LDS-tiled, 2 direct streaming (dwv_kernel)
  int pd;                 // dwv_kernel: input rows prefetched ahead (0: table / 1)
};
hipError_t dwk(const DwkArgs& a, hipStream_t s);
void dwk_tiles(const DwkArgs& a, int* cg, int* rb, int* tw, int* ntiles);
int dwk_seg(const DwkArgs& a);
// What dwk() would launch for these arguments, without launching: dwk() itself launches from
// this plan, so the two cannot disagree. hipErrorInvalidValue where dwk() refuses.
struct DwkPlan {
  int algo;               // 1 LDS-tiled (dwk_kernel), 2 direct streaming (dwv_kernel)
  int cb;                 // algo 1: CG, 8-channel chunks per workgroup; algo 2: CB, 4-channel chunk lanes
  int rb, tw, seg;        // output rows per band, output columns per tile (algo 2: 0), columns per item
  int pd;                 // algo 2: input rows prefetched ahead (algo 1: 0)
  int ntiles;             // pool parts per image; the grid is B * ntiles workgroups
  long lds;               // LDS bytes per workgroup
};
hipError_t dwk_plan(const DwkArgs& a, DwkPlan* p);

// Squeeze-excite tail: scale[b][c] = sigmoid(W2 SiLU(sum_parts pool / HW + b1) + b2).
struct SeArgs {
  const float* pool;      // [B][ntiles][Cs] fc1 partials from dwk
  const float* b1;        // [Cs]
  const float* w2t;       // [Cs][C] (fc2 transposed)
  const float* b2;        // [C]
  float* scale;           // [B][C]
  int B, ntiles, HW, C, Cs;
};
hipError_t squeeze_excite(const SeArgs& a, hipStream_t s);

struct ChScaleArgs {
  uint16_t* y;            // [B][HW][C] bf16, scaled in place
  const float* scale;     // [B][C]
  int B, HW, C;
};
hipError_t channel_scale(const ChScaleArgs& a, hipStream_t s);

// FP8 (OCP e4m3) GEMM, gemm_f8.hip: y = act(colscale[n] * A8 W8^T + bias[n]) (+res), bf16 or fp8 out.
struct GemmF8Args {
  const uint8_t* x;       // A e4m3 [M][ldx bytes]
  const uint8_t* wp;      // packed e4m3 [NF][K/128][2][64][16]
  const float* bias;      // [NF*16]
  const float* colscale;  // [NF*16] = s_a * s_w[n]
  const uint16_t* res;    // optional bf16 residual [M][ldr]
  uint16_t* y;            // bf16 out [M][ldy] (used when y8 is null)
  uint8_t* y8;            // e4m3 out [M][ldy], value / out_scale
  float out_inv_scale;
  int M, K, ldx, ldy, ldr, NF, nstore, relu_out;
  int krot;               // 1: each M tile starts its K loop at its own 128-deep step (env KDL_F8_KROT overrides)
};
hipError_t gemm_f8(int cfg, const GemmF8Args& a, hipStream_t s);
int gemm_f8_config(int cfg, int* bm, int* bn, int* threads);

// Classifier head: GAP over HW -> dense(F->H1)+ReLU -> dense(H1->NC), fp32 logits.
struct HeadArgs {
  const uint16_t* x;      // [B][HW][ldx] bf16
  const float* w1;        // [H1][F] fp32 (the Keras [F][H1] Dense kernel, transposed at load)
  const float* b1;        // [H1]
  const float* w2;        // [H1][NC]
  const float* b2;        // [NC]
  float* out;             // [B][NC]
  float* feat;            // scratch [B][F] fp32 (pooled features)
  float* hid;             // scratch [F/64][B][H1] fp32 (dense1 K-split partials)
  int B, HW, ldx, F, H1, NC;   // F multiple of 64, ldx >= F multiple of 8, H1 <= 128,
                               // (H1 + H1*NC + 256) floats of LDS within 64 KB
};
hipError_t head_dense(const HeadArgs& a, hipStream_t s);

// Classification outputs (kernels/classify.hip): per image, the K largest of its NC fp32
// logits and their softmax scores. Classes order by descending logit, equal logits by
// ascending index (TF top_k's rule); score_i = exp(x_i - max) / sum_j exp(x_j - max) over all
// NC logits, summed in a fixed order (replays are bit-identical). Output row: 2K 32-bit words,
// K int32 indices then K fp32 scores. 1 <= K <= min(NC, 32), 1 <= NC <= 1024 (kTopkMaxNC: 16
// logits per lane of a wave), ldx >= NC; anything else is hipErrorInvalidValue. NaN logits and
// a row that is entirely -inf give unspecified rows.
constexpr int kTopkMaxNC = 1024;
constexpr int kTopkMaxK = 32;
struct TopkArgs {
  const float* x;         // [B][ldx] fp32 logits, NC used per row
  int32_t* out;           // [B][2K]
  int B, NC, K, ldx;
};
hipError_t softmax_topk(const TopkArgs& a, hipStream_t s);

// Pooled-feature embeddings (kernels/embed.hip): out[b][c] = (1/HW) sum_p x[b][p][c] for the F
// channels of each image, accumulated in fp32 in a fixed order (replays are bit-identical).
// norm = 1: each row is then divided by max(||row||_2, 1e-12), torch.nn.functional.normalize's
// rule: an all-zero row stays zero. HW = 1 is a cast of one row (the ViT class token).
// F % 8 == 0, 8 <= F <= 4096 (kEmbedMaxF: 16 values per thread of the norm's workgroup),
// ldx % 8 == 0, ldx >= F, ldo >= F, x 16-byte aligned, 1 <= B <= 65535, HW >= 1, dt and norm
// 0 or 1; anything else is hipErrorInvalidValue and nothing is launched. Columns F..ldo of
// out are not written. One launch, two with norm. (EmbedArgs is the ViT token embedding's.)
constexpr int kEmbedMaxF = 4096;
struct EmbedRowsArgs {
  const uint16_t* x;      // [B][HW][ldx] bf16 / fp16, F used per pixel
  float* out;             // [B][ldo] fp32, F written per row
  int B, HW, F, ldx, ldo;
  int dt;                 // element type of x: 0 bf16, 1 fp16
  int norm;               // 0 raw mean, 1 L2-normalised
};
hipError_t embed_rows(const EmbedRowsArgs& a, hipStream_t s);

// Gallery search (kernels/similar.hip): score[b][j] = sum_i q[b][i] * g[j][i] of B fp32 query
// rows (an embed_rows output) against N stored bf16 rows, and per query the K best rows: by
// descending computed score, equal scores by ascending row index (softmax_topk's rule). Output
// row: 2K 32-bit words, K int32 row indices then K fp32 scores (TopkArgs' layout). The bf16
// values are taken as they stand and the query as fp32 (three bf16 terms per value on the
// matrix cores, fp32 accumulation): |score - exact| <= (F + 16) * 2^-23 * sum_i |q_i| * |g_ji|.
// Every row's sum runs in the same order, so equal rows give bit-equal scores and replays are
// bit-identical. Three launches: a small one splits the queries into their bf16 terms in `work`,
// a scan in which each workgroup keeps the K best of its kGalleryChunk rows in `work`, then a
// merge with one wave per query. The gallery is read once
// for B <= 32 and once per further 32 queries. Nothing is loaded past row N - 1 or column F - 1;
// pad columns of q and g are not read and out is written 2K words per row.
// F % 8 == 0, 8 <= F <= kEmbedMaxF, ldg % 8 == 0, ldg >= F, ldq >= F, 1 <= K <= min(N, kTopkMaxK),
// 1 <= N <= kGalleryMaxN, 1 <= B <= 1024, g and work 16-byte aligned; anything else is
// hipErrorInvalidValue and nothing is launched. NaN in q gives unspecified rows.
constexpr int kGalleryMaxN = 1 << 24;
constexpr int kGalleryChunk = 256;   // gallery rows per workgroup of the scan
struct GalleryTopkArgs {
  const float* q;         // [B][ldq] fp32 query rows, F used per row
  const uint16_t* g;      // [N][ldg] bf16 gallery rows, F used per row, 16-byte aligned
  int32_t* out;           // [B][2K]
  void* work;             // split queries + partial candidates: gallery_topk_workspace(B, N, K) bytes, 16-byte aligned
  int B, N, F, K, ldq, ldg;
};
size_t gallery_topk_workspace(int B, int N, int K);
hipError_t gallery_topk(const GalleryTopkArgs& a, hipStream_t s);

// Grad-CAM heatmaps (kernels/explain.hip): for each image the map of its predicted class,
//   raw_p = (1/HW) sum_c d_c x[b][p][c],   d_c = dlogit_k / d(mean_p x[b][p][c]),   k = top[b][0],
// with d in closed form for the two head kinds (no backward pass):
//   head = 0, linear  logit = W g + b:                  d_c = w[k][c]
//   head = 1, MLP     logit = relu(g W1 + b1) W2 + b2:  d_c = sum_j [z_j > 0] w2[j][k] w1[j][c], j ascending,
//     z_j = b1[j] + (even K-split partials of hid) + (odd ones), dense2_kernel's own order, so the
//     mask is the one the logits were computed with; z_j == 0 counts as off (torch's ReLU gradient).
// Output row, ldo fp32 words: word 0 the class (int32 bits) and word 1 the score, both copied
// from `top`; words 2 .. 2 + HW the map in the pixel order of x: max(raw_p, 0) for norm = 0, and for
// norm = 1 that value divided (a real fp32 division) by the row's largest, all zeros when the
// largest is 0. Columns past 2 + HW are not written. A class outside [0, NC) gives a zero map
// and reads nothing of w / w2. Sums run in fp32 in a fixed order: launches are bit-identical.
// `alpha` is an fp32 workspace [B][F] that receives d of the MLP head (the linear head's d is a
// row of w, read in place). One launch for the linear head, two for the MLP head, one more with norm.
// x, alpha and w 16-byte aligned, every other pointer aligned to its element and not null (the MLP
// pointers only for head = 1, w only for head = 0); F % 8 == 0 (linear) or F % 64 == 0 (MLP),
// 8 <= F <= kClassMapMaxF, 1 <= HW <= kClassMapMaxHW (16 values per thread of the norm's workgroup),
// 1 <= NC <= kClassMapMaxNC, 1 <= H1 <= kClassMapMaxH1 (head_dense's limit), 1 <= B <= 65535,
// ldx % 8 == 0, ldx >= F, ldo >= 2 + HW, dt / head / norm 0 or 1; anything else is
// hipErrorInvalidValue and nothing is launched.
constexpr int kClassMapMaxF = 4096;
constexpr int kClassMapMaxHW = 4096;
constexpr int kClassMapMaxNC = 1 << 20;
constexpr int kClassMapMaxH1 = 128;
struct ClassMapArgs {
  const uint16_t* x;      // [B][HW][ldx] bf16 / fp16, F used per pixel
  const int32_t* top;     // [B][2]: int32 class, fp32 score (a softmax_topk K = 1 row)
  const uint16_t* w;      // head 0: [NC][F] in the element type of x, 16-byte aligned
  const float* w1;        // head 1: [H1][F] (HeadArgs' layout)
  const float* w2;        // head 1: [H1][NC]
  const float* b1;        // head 1: [H1]
  const float* hid;       // head 1: [F/64][B][H1], the partials head_dense left behind
  float* alpha;           // workspace [B][F], 16-byte aligned (written for head 1)
  float* out;             // [B][ldo]
  int B, HW, F, ldx, ldo, NC, H1;
  int dt;                 // element type of x and w: 0 bf16, 1 fp16
  int head;               // 0 linear, 1 MLP
  int norm;               // 0 max(raw, 0), 1 divided by the row's maximum
};
hipError_t class_map(const ClassMapArgs& a, hipStream_t s);

// Attention rollout (kernels/rollout.hip; Abnar & Zuidema 2020): one launch per encoder layer next
// to its attention step, on the same packed qkv [B*T][3*H*dh] bf16. With P_h = softmax over the keys
// of Q_h K_h^T * scale (bf16 MFMA, fp32 accumulation, the full-row maximum and sum),
//   A^ = (mean_h P_h + I) / 2   (its rows sum to 1),   r_out = A^ r_in,   r_in == null: r_out = A^.
// r_in / r_out are fp32 [B][T][ldr]; the state and the product are fp32 throughout
// (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain). Only the query rows 0 .. Tq-1 are computed and
// written (the last layer needs row 0 alone); columns >= T, rows >= Tq and images >= B of r_out
// are never written, rows >= T of r_in never read and its columns >= T never used, keys >= T masked. Sums run in a
// fixed order without atomics: launches are bit-identical, row 0 of a Tq = 1 launch equals row 0
// of a Tq = T launch, and r_in == null equals an explicit identity r_in, bit for bit.
// dh != 64, T outside 1..kRolloutMaxT, H < 1, B < 1, Tq outside 1..T, ldr < T, ldr % 4 != 0, a null
// or not 16-byte aligned qkv / r_out (r_in: aligned when set) and r_in == r_out are
// hipErrorInvalidValue, and nothing is launched.
constexpr int kRolloutMaxT = 256;
struct AttnRolloutArgs {
  const uint16_t* qkv;
  const float* r_in;      // null: the first layer
  float* r_out;
  int B, T, Tq, H, dh;    // dh = 64
  float scale;            // 1/sqrt(dh)
  int ldr;                // row stride of r_in / r_out in floats
};
hipError_t attn_rollout(const AttnRolloutArgs& a, hipStream_t s);

// The rollout heatmap row of each image: out[b][0], out[b][1] = top[b] (int32 class, fp32 score: a
// softmax_topk K = 1 row), out[b][2 .. T] = r[b][0][1 .. T-1] divided (a real fp32 division) by
// their largest value: ClassMapArgs' row layout with h * w = T - 1. Columns past T are not written.
// T outside 2..kRolloutMaxT, B < 1, ldr < T, ldr % 4 != 0, ldo < T + 1 and a null or unaligned r /
// top / out are hipErrorInvalidValue, and nothing is launched.
struct RolloutMapArgs {
  const float* r;         // [B][T][ldr], row 0 of each image is read
  const int32_t* top;     // [B][2]
  float* out;             // [B][ldo]
  int B, T, ldr, ldo;
};
hipError_t rollout_map(const RolloutMapArgs& a, hipStream_t s);

// Rendered heatmap overlays (kernels/overlay.hip): behind class_map / rollout_map, one launch paints
// each image's h x w map over the S x S x 3 uint8 picture the model saw, in integers throughout
// (kdl/serving/overlay.py overlay_rule is the definition):
//   q[p]  = rint(min(max(heat[p], 0), 1) * 255), one fp32 multiply, round-half-even, NaN -> 0
//   u     = q resampled from h x w to S x S as Pillow's Image.resize does on an "L" image: the
//           horizontal pass, then the vertical one, runtime/resample.h's arithmetic (22-bit
//           coefficients, a uint8 intermediate, accumulators from 1 << 21) over the tables
//           resample_coeffs(w, S, filter) / resample_coeffs(h, S, filter)
//   c     = tab[u] (256 x 3 uint8, any colour table)
//   a_p   = a (blend 0, flat) or (a * u + 127) / 255 (blend 1, heat-weighted)
//   out   = (img * (256 - a_p) + c * a_p + 128) >> 8 per byte
// heat is read from the image's own output row, out[b][2 .. 2 + h*w) (ClassMapArgs' layout), and the
// picture's S*S*3 bytes are written behind it from word 2 + h*w on. Nothing else is written: words
// 0 .. 2 + h*w of a row, the pad bytes of the picture's last word, the words past it up to ldo and
// rows >= B stay as they were. Nothing outside [inp, inp + B*S*S*3) is read of the input, whose
// images sit at any byte alignment (it is read as aligned dwords, by bytes at its two ends).
// Launches are bit-identical. inp / out / tab / xb / xk / yb / yk / h_xb / h_yb null, out or a
// device table (tab, xb, xk, yb, yk) not 16-byte aligned, B outside 1..65535, h < 1, w < 1, h*w >
// kClassMapMaxHW, S < max(h, w), S > kOverlayMaxS, ldo < 2 + h*w + ceil(S*S*3 / 4), a outside
// 0..256, blend not 0 or 1, xks / yks outside 1..kOverlayMaxTaps, and bounds tables (checked from
// the host copies h_xb / h_yb, as resample.hip checks its own) whose taps leave the map, step
// back, or need more than kOverlayMaxRows map rows for one band of kOverlayBand output rows (no
// upscale does) are hipErrorInvalidValue, and nothing is launched.
constexpr int kOverlayMaxS = 1024;
constexpr int kOverlayMaxTaps = 8;
constexpr int kOverlayBand = 8;
constexpr int kOverlayMaxRows = 16;
struct HeatOverlayArgs {
  const uint8_t* inp;     // [B][S][S][3] uint8, packed
  float* out;             // [B][ldo] words: class, score, h*w heat values (read), the picture (written)
  const uint8_t* tab;     // 256 x 3 colour table
  const int32_t* xb;      // device: bounds [S][2] of the columns, {first map column, taps}
  const int32_t* xk;      // device: coefficients [S][xks]
  const int32_t* yb;      // device: the same of the rows
  const int32_t* yk;      // device: [S][yks]
  const int32_t* h_xb;    // HOST copies of the bounds (checked here, never followed on the device)
  const int32_t* h_yb;
  int B, S, h, w, ldo;
  int xks, yks;           // taps per column / row of the tables
  int a;                  // round(alpha * 256), 0..256
  int blend;              // 0 flat, 1 weighted by the heat
};
hipError_t heat_overlay(const HeatOverlayArgs& a, hipStream_t s);

// Dominant colours (kernels/palette.hip): behind class_map / rollout_map, two launches answer each
// image's K dominant colours, the picture's histogram weighted by its own heatmap and clustered, in
// integers throughout (kdl/serving/palette.py palette_rule is the definition):
//   w     = u >> 4 with u the map upsampled as heat_overlay does (weight 1), or 15 (weight 0, uniform)
//   bin   = (r >> 4) << 8 | (g >> 4) << 4 | (b >> 4); per bin n = sum w, sr / sg / sb = sum w * channel
//   W     = sum n; m = (s + n / 2) / n per live bin; K start centres by largest n, then largest
//           n * (squared distance to the nearest centre chosen), ties to the lowest bin; T rounds of
//           assign (ties to the lowest centre) and c = (S + N / 2) / N from the clusters' true sums;
//           sorted by N descending, ties to the lower centre
// heat is read from the image's own output row, out[b][2 .. 2 + h*w), and 1 + 2K words are written
// behind it: W, then K x (r | g << 8 | b << 16, N); centres that do not exist are 0, 0. Nothing else
// is written: the words before and after them up to ldo and rows >= B stay as they were. `work` is
// palette_workspace(B) bytes, all zero before the first launch; the second launch leaves it zero
// again. Every sum is an integer, so launches are bit-identical whatever the order of the atomics.
// inp / out / work / xb / xk / yb / yk / h_xb / h_yb null, out, work or a device table not 16-byte
// aligned, B outside 1..65535, h < 1, w < 1, h*w > kClassMapMaxHW, S < max(h, w), S > kOverlayMaxS
// (the uint32 bound: 15 * 255 * S*S + 15 * S*S / 2 < 2^32), ldo < 2 + h*w + 1 + 2K, K outside
// 1..kPaletteMaxK, T outside 1..kPaletteMaxT, weight not 0 or 1, xks / yks outside
// 1..kOverlayMaxTaps, and bounds tables (checked from the host copies) whose taps leave the map, step
// back, or need more than kOverlayMaxRows map rows for kOverlayBand output rows are
// hipErrorInvalidValue, and nothing is launched.
constexpr int kPaletteBins = 4096;
constexpr int kPaletteMaxK = 8;
constexpr int kPaletteMaxT = 16;
struct PaletteArgs {
  const uint8_t* inp;     // [B][S][S][3] uint8, packed
  float* out;             // [B][ldo] words: class, score, h*w heat values (read), W and K x (colour, N) (written)
  uint32_t* work;         // [B][kPaletteBins][4] sums, zero on entry and on exit
  const int32_t* xb;      // device: bounds [S][2] of the columns, {first map column, taps}
  const int32_t* xk;      // device: coefficients [S][xks]
  const int32_t* yb;      // device: the same of the rows
  const int32_t* yk;      // device: [S][yks]
  const int32_t* h_xb;    // HOST copies of the bounds (checked here, never followed on the device)
  const int32_t* h_yb;
  int B, S, h, w, ldo;
  int xks, yks;           // taps per column / row of the tables
  int K, T;               // colours, rounds
  int weight;             // 0 uniform (15), 1 the map (u >> 4)
};
size_t palette_workspace(int B);
hipError_t palette(const PaletteArgs& a, hipStream_t s);

// Garment boxes (kernels/locate.hip): behind class_map / rollout_map, two launches answer each image's K
// largest connected regions of its own heatmap, in integers throughout (kdl/serving/locate.py
// locate_rule is the definition):
//   mask  = u >= threshold with u the map upsampled as heat_overlay does
//   8-connected components; a component's identity is its first pixel in raster order
//   count = all components; the K largest by pixel count, ties to the earlier first pixel
// heat is read from the image's own output row, out[b][2 .. 2 + h*w), and 1 + 3K words are written
// behind it: count, then K x (y0 | x0 << 16, y1 | x1 << 16, area), y1 and x1 exclusive; boxes that do
// not exist are 0, 0, 0. Nothing else is written: the words before and after them up to ldo and rows
// >= B stay as they were. The picture is never read. `work` is locate_workspace(B, S) bytes; every
// launch writes all it reads of it first (the bitmask whole, the run tables up to the image's run
// count), so a replay needs nothing from the host and the content before a launch does not matter.
// Per image it holds the bitmask, S rows of ceil(S / 64) 64-bit words, and, where S * ceil(S / 2) >
// kLocateLdsRuns, three uint32 tables of S * ceil(S / 2) runs: S*S/8 + 6*S*S bytes, 6.2 per pixel.
// The result does not depend on the order of the atomics or on the schedule.
// out / work / xb / xk / yb / yk / h_xb / h_yb null, out, work or a device table not 16-byte aligned,
// B outside 1..65535, h < 1, w < 1, h*w > kClassMapMaxHW, S < max(h, w), S > kOverlayMaxS (coordinates
// in 16 bits), ldo < 2 + h*w + 1 + 3K, K outside 1..kLocateMaxK, threshold outside 1..255, xks / yks
// outside 1..kOverlayMaxTaps, and bounds tables (checked from the host copies) whose taps leave the
// map, step back, or need more than kOverlayMaxRows map rows for kOverlayBand output rows are
// hipErrorInvalidValue, and nothing is launched.
constexpr int kLocateMaxK = 8;
constexpr int kLocateLdsRuns = 1920;   // an image with more runs keeps its run tables in `work`, not in LDS
struct LocateArgs {
  float* out;             // [B][ldo] words: class, score, h*w heat values (read), count and K x (corner, corner, area) (written)
  uint8_t* work;          // locate_workspace(B, S) bytes
  const int32_t* xb;      // device: bounds [S][2] of the columns, {first map column, taps}
  const int32_t* xk;      // device: coefficients [S][xks]
  const int32_t* yb;      // device: the same of the rows
  const int32_t* yk;      // device: [S][yks]
  const int32_t* h_xb;    // HOST copies of the bounds (checked here, never followed on the device)
  const int32_t* h_yb;
  int B, S, h, w, ldo;
  int xks, yks;           // taps per column / row of the tables
  int K;                  // boxes
  int threshold;          // 1..255 of the upsampled map
};
size_t locate_workspace(int B, int S);
hipError_t locate(const LocateArgs& a, hipStream_t s);

// Garment cutouts (kernels/cutout.hip): behind class_map / rollout_map, three launches answer each image's
// picture with an alpha channel, in integers throughout (kdl/serving/cutout.py cutout_rule is the
// definition):
//   u = the map upsampled as heat_overlay does; ok = u >= gate
//   N, G, F over the 4096 colour bins of palette: pixels, gated pixels, the sum of u
//   rounds + 1 times: bin b is garment-coloured iff N > 0 and F * TB >= (255 N - F) * TF with TF = sum F,
//   TB = 255 S^2 - TF (64-bit products); F <- 255 G where it is, else 0
//   mask = fg[bin] & ok, then `smooth` 3 x 3 majority rounds (outside the picture counts as unset)
//   alpha = feather ? (255 c + 4) / 9 with c the set pixels of the 3 x 3 window : 255 mask
// heat is read from the image's own output row, out[b][2 .. 2 + h*w), and 1 + S*S words are written behind
// it: the garment's pixel count, then r | g << 8 | b << 16 | alpha << 24 per pixel. Nothing else is
// written: the words before and after them up to ldo and rows >= B stay as they were. `work` is
// cutout_workspace(B, S) bytes: per image the three tables (zero on entry and on exit), the 4096 colour
// bits and the gate's bitmask, S rows of ceil(S / 64) 64-bit words; the bits and the mask are written whole
// by every launch before they are read, so a replay needs nothing from the host. The result does not depend
// on the order of the atomics or on the schedule.
// inp / out / work / xb / xk / yb / yk / h_xb / h_yb null, out, work or a device table not 16-byte aligned,
// B outside 1..65535, h < 1, w < 1, h*w > kClassMapMaxHW, S < max(h, w), S > kOverlayMaxS (the uint32
// tables), ldo < 2 + h*w + 1 + S*S, gate outside 1..255, rounds outside 0..kCutoutMaxRounds, smooth outside
// 0..kCutoutMaxSmooth, feather not 0 or 1, xks / yks outside 1..kOverlayMaxTaps, and bounds tables (checked
// from the host copies) whose taps leave the map, step back, or need more than kOverlayMaxRows map rows
// for kOverlayBand output rows are hipErrorInvalidValue, and nothing is launched.
constexpr int kCutoutMaxRounds = 8;
constexpr int kCutoutMaxSmooth = 4;
struct CutoutArgs {
  const uint8_t* inp;     // [B][S][S][3] the pictures the model saw
  float* out;             // [B][ldo] words: class, score, h*w heat values (read), count and S*S RGBA words (written)
  uint8_t* work;          // cutout_workspace(B, S) bytes, the tables of every image zero
  const int32_t* xb;      // device: bounds [S][2] of the columns, {first map column, taps}
  const int32_t* xk;      // device: coefficients [S][xks]
  const int32_t* yb;      // device: the same of the rows
  const int32_t* yk;      // device: [S][yks]
  const int32_t* h_xb;    // HOST copies of the bounds (checked here, never followed on the device)
  const int32_t* h_yb;
  int B, S, h, w, ldo;
  int xks, yks;           // taps per column / row of the tables
  int gate;               // 1..255 of the upsampled map
  int rounds;             // re-estimates of the colour model behind the first
  int smooth;             // majority rounds
  int feather;            // 1 = alpha is the 3 x 3 mean of the mask
};
size_t cutout_workspace(int B, int S);
hipError_t cutout(const CutoutArgs& a, hipStream_t s);

// Baseline JPEG encode (kernels/jpeg_encode.hip): B pictures uint8 [H][W][3], picture b at inp + b * ldi
// bytes (any alignment), each into the file Pillow's Image.save(.., "JPEG", quality, subsampling,
// optimize=False) writes, byte for byte (kdl/serving/jpeg_encode.py encode_rule is the definition:
// libjpeg's fixed-point colour, h2v2 average, islow DCT, Annex K tables, one interleaved scan).
// Output row b, ldo words: nfront words copied from front[b * ldf ..] (nfront = 0: none), one word with
// the file's length in bytes, then the file and zero bytes up to ceil(cap / 4) words. A file longer
// than cap gives length 0 and nothing is written behind the length word of that row; other rows are
// unaffected. Words past nfront + 1 + ceil(cap / 4) of a row and rows >= B are not written.
// The first kJpegHeaderBytes bytes of every file are `hdr` (device), whose quantisation tables the
// kernels use; h_hdr is the host copy, checked here against H, W, quality and sampling. Four launches:
// coefficients per MCU row, bit offsets per picture, the bits ORed into the picture's zeroed stream
// (the kernels clear what they OR into, every launch), byte stuffing and the row. OR is commutative
// and every sum is an integer: launches are byte-identical.
// inp / hdr / h_hdr / out / work null (front: only with nfront > 0), out / front / work not aligned to
// 4 / 4 / 16 bytes, B outside 1..65535, H or W outside 1..kJpegEncMaxSide, quality outside 1..100,
// sampling not 0 (4:4:4) or 1 (4:2:0), cap outside 1..kJpegEncMaxCap, ldi < H*W*3, nfront < 0,
// ldf < nfront, ldo < nfront + 1 + ceil(cap / 4), or a header that is not the one of these arguments
// are hipErrorInvalidValue, and nothing is launched.
constexpr int kJpegHeaderBytes = 623;
constexpr int kJpegEncMaxSide = 1024;
constexpr int kJpegEncMaxCap = 1 << 24;
struct JpegEncodeArgs {
  const uint8_t* inp;     // pictures [H][W][3], packed rows; picture b at inp + b * ldi
  const uint8_t* hdr;     // device: the kJpegHeaderBytes bytes in front of the scan
  const uint8_t* h_hdr;   // HOST copy of hdr (checked here, never followed on the device)
  const uint32_t* front;  // [B][ldf] words in front of each row's length word, or null
  uint32_t* out;          // [B][ldo] words
  void* work;             // jpeg_encode_workspace(B, H, W, sampling, cap) bytes, 16-byte aligned
  int64_t ldi;            // bytes between pictures
  int B, H, W, quality, sampling, cap, ldo, nfront, ldf;
};
size_t jpeg_encode_workspace(int B, int H, int W, int sampling, int cap);
hipError_t jpeg_encode(const JpegEncodeArgs& a, hipStream_t s);

// PIL-exact NEAREST resize of one uint8 HWC RGB image into slot `b` of a
// [B][OH][OW][3] uint8 batch, using host-built index tables.
struct ResizeArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int* ytab;        // [OH] source rows
  const int* xtab;        // [OW] source cols
  int SH, SW, OH, OW;
  int n;                  // images of one source size, packed [n][SH][SW][3] -> [n][OH][OW][3] (0 = 1)
};
hipError_t resize_nearest_u8(const ResizeArgs& a, hipStream_t s);

// Baseline JPEG pixel work (kernels/jpeg.hip): the host has entropy-decoded n images into
// coefficient planes (runtime/jpeg.h); jpeg_idct_u8 makes uint8 sample planes of all of them,
// jpeg_sample_rgb_u8 gathers each image's resized RGB into row desc.out_row of out. Both
// launchers check every descriptor (the host copy) against the capacities given here.
struct JpegDesc;
struct JpegArgs {
  const JpegDesc* desc;     // [n] in device memory
  const JpegDesc* h_desc;   // the same [n] in host memory (checked, never dereferenced on the device)
  const int16_t* coef;      // coefficients, coef_cap int16
  const uint16_t* qt;       // quantisation tables, natural order, qt_cap uint16
  uint8_t* planes;          // sample-plane scratch, plane_cap bytes
  uint8_t* out;             // [out_rows][OH][OW][3]
  uint64_t coef_cap, plane_cap;
  int qt_cap, n, n_wg, out_rows, OH, OW;
};
hipError_t jpeg_idct_u8(const JpegArgs& a, hipStream_t s);
hipError_t jpeg_sample_rgb_u8(const JpegArgs& a, hipStream_t s);

// Baseline JPEG entropy decode (kernels/jpeg_huff.hip): the host has staged each image's Huffman
// tables and unstuffed scan (jpeg_scan_prepare, runtime/jpeg_huff.h); jpeg_huff_decode clears the
// image's coefficient planes and Huffman-decodes the scan into them (AC values, DC differences),
// jpeg_dc_scan sums the DC differences. The planes are then what jpeg_idct_u8 reads. Both
// launchers check every descriptor (the host copy) against the capacities given here.
struct JpegHuffDesc;
struct JpegHuffArgs {
  const JpegHuffDesc* desc;    // [n] in device memory
  const JpegHuffDesc* h_desc;  // the same [n] in host memory (checked, never dereferenced on the device)
  const uint8_t* stage;        // tables and scans, stage_cap bytes
  int16_t* coef;               // coefficients, coef_cap int16
  uint32_t* status;            // per image: error word (non-zero = ask the host decoder), most rounds of a chunk
  uint64_t stage_cap, coef_cap;
  int status_cap;              // uint32 of status: at least 2 * n
  int n;
  const uint8_t* h_stage;      // the restart launchers: the host's copy of stage (its tables are checked, see below)
};
hipError_t jpeg_huff_decode(const JpegHuffArgs& a, hipStream_t s);
hipError_t jpeg_dc_scan(const JpegHuffArgs& a, hipStream_t s);
// The same for files with restart intervals, whose descriptors carry an interval and a group table
// (runtime/jpeg_huff.h): one workgroup per (image, group of intervals), each from the known entry
// state of its intervals, and DC sums that start again at every interval. The workgroups of an
// image share its two status words: jpeg_huff_rst_decode clears them on the stream first.
hipError_t jpeg_huff_rst_decode(const JpegHuffArgs& a, hipStream_t s);
hipError_t jpeg_dc_rst_scan(const JpegHuffArgs& a, hipStream_t s);

// Pillow's filtered resize + crop (kernels/resample.hip): a table-driven separable convolution
// over uint8 RGB. resample_h_u8 runs the horizontal pass of n images into the intermediate
// scratch (kind 0: packed raw pixels; 1: the sample planes of jpeg_idct_u8), resample_v_u8 the
// vertical pass into each image's row desc.out_row of out. Both launchers check every descriptor
// and bounds table (the host copies) against the capacities given here.
struct ResampleDesc;
struct ResampleArgs {
  const ResampleDesc* desc;    // [n] in device memory
  const ResampleDesc* h_desc;  // the same [n] in host memory (checked, never dereferenced on the device)
  const JpegDesc* jdesc;       // kind 1: the call's JPEG descriptors, n_jdesc of them (device / host copy)
  const JpegDesc* h_jdesc;
  const uint8_t* planes;       // kind 1: sample planes, plane_cap bytes
  uint8_t* tmp;                // intermediate scratch, tmp_cap bytes
  uint8_t* out;                // [out_rows][OH][OW][3]
  uint64_t plane_cap, tmp_cap;
  int n_jdesc, n, out_rows, OH, OW;
};
hipError_t resample_h_u8(const ResampleArgs& a, int kind, hipStream_t s);
hipError_t resample_v_u8(const ResampleArgs& a, hipStream_t s);

// Elementwise: uint8 HWC image -> Xception-normalised bf16 NHWC padded to ldy
// (x/127.5 - 1), used by the non-folded path and by tests.
hipError_t u8_to_bf16_norm(const uint8_t* x, uint16_t* y, long npix, int ldy, hipStream_t s);

}  // namespace kdl
