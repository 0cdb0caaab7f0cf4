/* libmmd - C ABI of the MI355X-native MM-Diffusion denoising hot path.
 *
 * One shared library (mm-diffusion_amd/lib/libmmd.so, built by hipcc --offload-arch=gfx950) loaded with
 * ctypes by the Python host mirror (mm-diffusion_amd/mm_diffusion/_hip.py).  The reference has no native
 * layer (pure PyTorch), so each entry point replaces a GROUP of ATen calls of the reference hot path; the
 * reference interface it replaces is cited per function (paths relative to /root/reference/mm_diffusion).
 *
 * Conventions
 *   - raw DEVICE pointers + sizes; row-major "channels-last" activations X[rows, C] with a row stride `ld`
 *     in ELEMENTS (so a column slice of a wider buffer is a valid tensor: skip concats are free views);
 *     video rows are ordered (n, f, h, w), audio rows (n, l)
 *   - dtype: MMD_F32 (0) or MMD_BF16 (1) = element type of activations / GEMM weights; all statistics,
 *     accumulation, softmax and bias arithmetic are fp32
 *   - every call only ENQUEUES work on `stream` (a hipStream_t); no allocation, no sync: the caller owns all buffers including
 *     workspaces; calls are re-entrant and graph-capturable.  Global state: the dynamic-LDS size granted to each kernel, per device
 *     (raised at the first launch that needs more, so a launch sequence that has run once sets nothing when repeated), and the values
 *     of the tuning / A-B switches of the environment (INTEGRATION.md section 4 has the table; read through mmd_env_int / mmd_env_char /
 *     mmd_env_set of mmd_common.h) - MMD_VCONV_RING at every call; once per process, at first use: MMD_GN_BLOCKS, MMD_STRIP_BLOCKS, MMD_STRIP_K128_RF1, MMD_GEMM_DESC, MMD_TCONV_BLOCKS, MMD_STEM_MFMA, MMD_ATTN_DMA,
 *     MMD_ATTN_PIPE, MMD_ATTN_PIPE_LDSPAD, MMD_WGRAD_TR, MMD_WGRAD_TILE64, MMD_WGRAD_BLOCKS
 *   - return 0 on success, <0 on error (MMD_ERR_*); mmd_last_error() gives the message (thread local)
 *
 * Size limits.  Row counts are int (M < 2^31); what can grow past 32 bits is the BYTE range of a strided operand, (rows - 1) * ld * ES +
 * C * ES - a bf16 ds1 tensor of the base model passes 2 GiB at batch 43 and 4 GiB at batch 86.  Kernels address rows as int64 row * ld
 * unless listed here (tests/bigaddr.py holds the same table as data; tests/test_bigaddr_gpu.py runs both sides of every limit):
 *   - mmd_conv_gemm* / mmd_gn_conv1x1* tiles 129 and 132: a 32-bit buffer descriptor over A while (M * lda + Cin) * ES < 2 GiB, the
 *     64-bit pointer instantiation of the same loop beyond - same results, nothing refused
 *   - tile 133 (also through mmd_gn_conv_gemm): a descriptor per FRAME of A; a frame whose rows span 2 GiB or more is refused by name
 *     (tile 130 takes it and is bitwise equal: ops.halo_tile_code)
 *   - tile 131: Y and R by 32-bit byte offsets from the launch's base.  Rows whose offsets would pass 4 GiB are run as several launches
 *     of the same kernel, cut at multiples of 256 rows, of the GroupNorm slice and of the (D0, D1, D2) sample of a conv with taps, so
 *     the results - statistics records included - do not depend on it; only when ONE such unit of Y or R spans 4 GiB (row strides
 *     of megabytes) is the launch refused by name (ops.strip_tile_ok knows)
 *   - mmd_gn_conv1x1_skip: M * ldy * 2 < 4 GiB, refused by name beyond (ops.skip_fusable knows; the two launches it replaces run instead)
 *   - mmd_attn_fwd impl 4 / 5 (and 0 at head width 64): a descriptor over the K/V rows of the batches of one launch; batches are cut into
 *     launches of less than 2 GiB of K/V; ONE batch of 2 GiB or more is refused for impl 4 / 5 and runs the per-128-query kernel (bitwise
 *     equal) for impl 0.  Q and O are 64-bit
 *   - mmd_vconv2d1d: one SAMPLE's rows of X below 2 GiB (a descriptor re-based per sample), refused by name beyond (ops.vconv_shape_ok)
 *   - mmd_conv_wgrad: the transposing 9-tap kernel while M * ld * 2 < 2 GiB on both operands, the 128-tile kernel beyond
 *   No other entry has a limit on a strided activation: they form int64 row * ld (the buffer descriptors in mmd_tconv, mmd_tattn_block and
 *   mmd_vconv2d1d's second one cover the packed weight image only), and every strided entry is run at ranges past 2 and 4 GiB by
 *   tests/test_bigaddr_gpu.py - also with the extent carried by a Geom's outer_stride or tstride alone.
 */
#ifndef MMD_H
#define MMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MMD_F32 0
#define MMD_BF16 1
#define MMD_OK 0
#define MMD_ERR_ARG (-1)
#define MMD_ERR_LAUNCH (-2)
#define MMD_ERR_UNSUPPORTED (-3)

int mmd_version(void);
const char* mmd_last_error(void);
/* test-suite aid: print the native backtrace of a fatal signal (SIGSEGV / SIGBUS / SIGABRT) to stderr, then chain to the handler
 * installed before (Python's faulthandler).  Never called by the product path. */
int mmd_debug_install_crash_handler(void);

/* --- HIP graph capture of one denoising step + stream-ordered timing (bench roofline leg) --- */
int mmd_graph_begin(void* stream);
int mmd_graph_end(void* stream, void** exec_out);
int mmd_graph_launch(void* exec, void* stream);
int mmd_graph_destroy(void* exec);
/* private launch streams of the host mirror (hipStreamNonBlocking): the video / audio chains and the capture stream */
int mmd_stream_create(void** stream_out);
int mmd_stream_sync(void* stream);
int mmd_stream_destroy(void* stream);
int mmd_event_create(void** ev);
int mmd_event_record(void* ev, void* stream);
int mmd_stream_wait_event(void* stream, void* ev);   /* fork/join of the video and audio launch streams (also under capture) */
int mmd_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);
int mmd_event_destroy(void* ev);

/* timestep_embedding + time_embed MLP (nn.py:192-210; multimodal_unet.py:791-795,1075).
 * t_kind: 0 int64, 1 int32, 2 float32.  out_silu[N,dim] = SiLU(time_embed(emb(t))) (the input every
 * ResBlock emb_layers applies its Linear to, unet:366-372); out_raw (nullable) = time_embed output. */
int mmd_temb_fwd(const void* t, int t_kind, int N, int dim, const float* W0, const float* b0, const float* W2,
                 const float* b2, float* out_silu, float* out_raw, void* stream);

/* y[N,J] = x[N,K] W[J,K]^T + b : all ResBlock emb_layers Linear(128 -> 2*Cout) batched into one call
 * over the row-concatenated weights (unet:366-372,454). */
int mmd_linear_fwd(const float* x, const float* W, const float* b, float* y, int N, int K, int J, void* stream);

/* GroupNorm32 statistics -> fused per-(slice,channel) affine (nn.py:16-33; FiLM unet:457-470).
 * Slice s normalises rows base(s) + j*tstride (j < Tn), base(s) = (s/inner)*outer_stride + (s%inner)*inner_stride.
 * a_out/b_out [S, C] fp32: y = x*a + b; mr_out (nullable) [S, 32, 2] = (mean, rstd) for the backward.  film (nullable) [S, >=2C] rows (scale | shift), row stride film_ld.
 * workspace: mmd_gn_workspace_bytes(dtype, C, S, Tn) bytes (may be 0: slice handled by one block). */
int64_t mmd_gn_workspace_bytes(int dtype, int C, int S, int Tn);
int mmd_gn_stats(int dtype, const void* x, int64_t ld, int C, int S, int Tn, int inner, int64_t outer_stride,
                 int64_t inner_stride, int64_t tstride, const float* gamma, const float* beta, const float* film,
                 int64_t film_ld, float eps, float* a_out, float* b_out, float* mr_out, void* workspace, void* stream);
/* The same fused affine from PRODUCER-side statistics: the GEMM that wrote x (mmd_conv_gemm_stats / mmd_gn_conv1x1_stats) left per
 * (64-row record, QUAD of 4 channels) float2 (sum, sum of squares) in rec[(row / 64) * rec_ld + quad]; rec points at the first quad of
 * the C normalised channels (C % 128 == 0: groups of whole quads); S contiguous slices of Tn rows, Tn % 64 == 0.
 * Replaces the statistics pass over x of GroupNorm32 (nn.py:16-33) for conv-fed norms. */
int mmd_gn_finalize_stats(const float* rec, int64_t rec_ld, int C, int S, int Tn, const float* gamma, const float* beta,
                          const float* film, int64_t film_ld, float eps, float* a_out, float* b_out, float* mr_out, void* stream);
/* y = act(x*a[slice(row)] + b[slice(row)]), act: 0 none, 1 SiLU (nn.SiLU after every GroupNorm32). */
int mmd_gn_apply(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int C, int S, int Tn, int inner,
                 int64_t outer_stride, int64_t inner_stride, int64_t tstride, const float* a, const float* b, int act,
                 void* stream);
/* x[m, :] += e[m / rows_per_sample, :]  (non-FiLM ResBlock h + emb_out, unet:473-477). */
int mmd_add_rowbias(int dtype, void* x, int64_t ld, int64_t rows, int C, int64_t rows_per_sample, const float* e,
                    int64_t e_ld, void* stream);
/* Its gradient w.r.t. e: out[s, c] += sum over the rows of sample s of dY[row, c] (S contiguous slices of Tn rows; out fp32 [S, ldo],
 * accumulated - the caller zeroes). */
int mmd_colsum_slices(int dtype, const void* dY, int64_t lddy, int S, int64_t Tn, int C, float* out, int64_t ldo, void* stream);

/* Implicit-GEMM convolution on the matrix cores:
 *   Y[m, co] = bias[co] + sum_tap sum_ci A[src(m,tap), ci] * W[co, tap*Cin + ci] (+ R[m, co])
 * rows m decompose as (n, p0, p1, p2) over (D0, D1, D2); tap t = taps[3t..3t+2] offsets (p0,p1,p2), out of
 * range -> zero padding.  Covers VideoConv 2d+1d spatial (D=(1,H,W), 9 taps) and temporal (D=(F,HW,1), 3 taps),
 * VideoConv '3d' k=1, AudioConv k=3 dilated (D=(L,1,1), taps (+-d,0,0)) and k=1, and every qkv/proj 1x1 conv
 * (unet:83-131,272,275,378,401,605-610).  W is [Cout][ntaps*Cin] in `dtype`; bias fp32 (nullable);
 * R (nullable) residual in `dtype`.  taps is a HOST pointer.  tile: 0 auto, 64 or 128 (register-staged
 * main loop), 129 (128x128 tile, direct-to-LDS global_load_lds main loop), 132 (129 with a four-slot LDS ring - three K steps of
 * DMA in flight, one block per CU - for launches with fewer tiles than the chip has block slots; Cin a multiple of 128 bytes),
 * 131 (bf16 convs with ntaps * Cin in {128, 256, 384, 512}: row strips stationary in registers, weights streamed through
 * LDS); these variants are bitwise identical.  130 = halo-tile
 * main loop for spatial 3x3 convs (chunk-major K order: equal to rounding); 133 = the same on 16 x 16 pixel patches (bf16, 8 waves,
 * one block per CU, three-slot weight ring; D1 % 16 == 0, D2 % 16 == 0), bitwise equal to 130. */
int mmd_conv_gemm(int dtype, const void* A, int64_t lda, const void* W, const float* bias, const void* R, int64_t ldr,
                  void* Y, int64_t ldy, int M, int Cout, int Cin, int ntaps, const int* taps, int D0, int D1, int D2, int tile,
                  void* stream);

/* 1x1 conv whose input GroupNorm32(+FiLM)(+SiLU) is applied on the way into LDS (no normalised tensor in HBM):
 *   Y = act(A * gn_a[s(m)] + gn_b[s(m)]) W^T + bias (+ R),  s(m) = m / rows_per_slice  (S contiguous slices, S*rows == M,
 *   rows_per_slice >= 128, Cin <= 256).  gn_a / gn_b [S, Cin] come from mmd_gn_stats.  Replaces the ResBlock tail
 *   norm -> SiLU -> out conv -> + skip (unet:373-388,457-483).  tile 131 (bf16): the normalisation is applied once per row
 *   strip in registers, so wide outputs (the qkv convs of the attention blocks, unet:272,605-606) fuse too; it needs
 *   rows_per_slice >= 256 (Cin 128 / 256) or >= 128 (Cin 384). */
int mmd_gn_conv1x1(int dtype, const void* A, int64_t lda, const float* gn_a, const float* gn_b, int act, int S,
                   int64_t rows_per_slice, const void* W, const float* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                   int M, int Cout, int Cin, int tile, void* stream);

/* GroupNorm32(+SiLU) of S SHORT slices (Tn <= 16 rows; geometry as mmd_gn_stats) in one launch and one read of the tensor: the
 * temporal-attention norm over the frames of a pixel (unet:489-490 -> nn.py:16-33) = mmd_gn_stats + mmd_gn_apply.  Exact two-pass
 * statistics on register-resident data; channel groups must be whole quads (C % 128 == 0). */
int mmd_gn_small(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int C, int S, int Tn, int inner, int64_t outer_stride,
                 int64_t inner_stride, int64_t tstride, const float* gamma, const float* beta, float eps, int act, void* stream);

/* GroupNorm32(+FiLM)(+SiLU) of slices of a few hundred rows in ONE launch (nn.py:16-33; FiLM unet:457-470): one block per (group, slice),
 * the group's Tn x C / 32 elements register-resident (Tn * C / 128 <= 4096), exact two-pass fp32 statistics.  Writes the fused affine
 * a_out / b_out [S, C] (nullable pair: as mmd_gn_stats), the normalised tensor y (nullable: as mmd_gn_apply; act: 0 none, 1 SiLU), or
 * both = mmd_gn_stats (two launches on multi-block slices) + mmd_gn_apply for the slices whose rows are no multiple of the 64-row
 * producer records (the 400-row audio samples at ds8).  Geometry, film, mr_out as mmd_gn_stats; C % 128 == 0. */
int mmd_gn_group(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int C, int S, int Tn, int inner, int64_t outer_stride,
                 int64_t inner_stride, int64_t tstride, const float* gamma, const float* beta, const float* film, int64_t film_ld,
                 float eps, int act, float* a_out, float* b_out, float* mr_out, void* stream);

/* hipMemsetAsync(ptr, 0, bytes) on the stream (a memset node of a captured plan). */
int mmd_zero(void* ptr, int64_t bytes, void* stream);

/* The two GEMMs above with the GroupNorm statistics of their OUTPUT produced in the epilogue, for the norm that consumes Y next
 * (ResBlock in_layers / out_layers norms, attention norms, the heads: unet:339-340,374-375; nn.py:16-33): per (64-row record,
 * QUAD of 4 consecutive columns) the sum and the sum of squares of the values as stored, stats[(m / 64) * stats_ld + quad] =
 * float2 (per column until round 3: every group size of the model is a multiple of 4 and the per-quad fold costs the producers a
 * third of the instructions).  `stats` points at the first quad this launch writes (producers of a channel-concatenated tensor
 * fill column slices of one record buffer); Cout % 4 == 0.
 * M % 64 == 0; not with tile 130; tile 131 emits them for every K it accepts (K = 128 / 256: a wave owns whole 64-row records;
 * K = 384 / 512: two waves' half-records are paired through LDS).  The order in which a record's 64 rows are folded belongs
 * to the kernel family (tiles 128 / 129 share one, 131 has its own): a layer must be given the same family at every batch size
 * if its results are to be batch-invariant to the last bit.  mmd_gn_finalize_stats consumes the records. */
int mmd_conv_gemm_stats(int dtype, const void* A, int64_t lda, const void* W, const float* bias, const void* R, int64_t ldr,
                        void* Y, int64_t ldy, int M, int Cout, int Cin, int ntaps, const int* taps, int D0, int D1, int D2, int tile,
                        float* stats, int64_t stats_ld, void* stream);
int mmd_gn_conv1x1_stats(int dtype, const void* A, int64_t lda, const float* gn_a, const float* gn_b, int act, int S,
                         int64_t rows_per_slice, const void* W, const float* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                         int M, int Cout, int Cin, int tile, float* stats, int64_t stats_ld, void* stream);

/* The ResBlock tail of a channel-changing block in ONE launch: out conv of the normalised h plus the 1x1 skip conv of x
 * (unet:373-388,401,457-483), on the row-strip kernel with two register-stationary operands:
 *   Y[m, :] = bf16( (W_out . g(h[m, :]) + bias_out) + float( bf16( W_skip . x[m, :] + bias_skip ) ) )
 *   g(h) = act(h * gn_a[s(m)] + gn_b[s(m)]) on the K1 channels of h only (gn_a / gn_b [S, K1]; act: 0 none, 1 SiLU); x is not normalised.
 * Bitwise equal to mmd_conv_gemm(x, W_skip, bias_skip) -> sk followed by mmd_gn_conv1x1[_stats](h, ..., R = sk, tile 131): the skip
 * product has its own accumulator (ascending k), gets its bias and is rounded to bf16 where sk would have been stored, and is added
 * where the residual is added; the two biases are never pre-added.  The tensor sk, its write, its read and one launch disappear.
 * stats (nullable) / stats_ld as mmd_gn_conv1x1_stats; the records are folded in the order of the one-fragment K = 128 strip
 * instance, which is what the two-launch path runs for slices of >= 16384 rows (with shorter slices that path's records differ
 * in the last bit, Y does not).  bf16; K1 == 128, K2 in {256, 384} (K1 + K2 <= 512: an argument error beyond), Cout % 32 == 0,
 * Cout <= 2048, rows_per_slice >= 128, S * rows_per_slice == M; pointers and row strides 16-byte multiples, M * ldy * 2 < 4 GB.
 * Any other shape returns MMD_ERR_UNSUPPORTED: no fallback inside the library. */
int mmd_gn_conv1x1_skip(int dtype, const void* h, int64_t ldh, const float* gn_a, const float* gn_b, int act, int S,
                        int64_t rows_per_slice, const void* W_out, const float* bias_out, const void* x, int64_t ldx, int K2,
                        const void* W_skip, const float* bias_skip, void* Y, int64_t ldy, int M, int Cout, int K1, float* stats,
                        int64_t stats_ld, void* stream);

/* The same ResBlock tail for the deeper levels, with K STREAMED instead of register-stationary (mmd_rtail.hip; the mapping of
 * mmd_aconv): Y[m, :] = bf16( (W . act(h[m, :] * ga[s] + gb[s]) + bias) + float( bf16( W2 . x[m, :] + bias2 ) ) ), s = m / L.
 * h [M, ldh] (K1 columns), x [M, ldx] (K2 columns), W [Cout][K1], W2 [Cout][K2] (mmd_conv_gemm's weight layout), ga / gb [M / L, K1]
 * fp32 or BOTH null (h is already normalised: the launch then runs behind mmd_gn_apply), act: 0 none, 1 SiLU (ignored without the
 * affine).  Bitwise equal - Y and the statistics records - to mmd_conv_gemm(x, W2, bias2) -> sk followed by the out conv the layer
 * runs on the row-strip tile (mmd_gn_conv1x1[_stats](h, ..., R = sk, tile 131), or mmd_gn_apply + mmd_conv_gemm[_stats](tile 131)):
 * the records are folded in that launch's order - one row fragment per wave at K1 >= 384 and at K1 = 128 with the affine and
 * L >= 16384, two fragments otherwise.  stats (nullable) / stats_ld as mmd_conv_gemm_stats (M % 64 == 0).
 * bf16; K1 in {128, 256, 384, 512}, K2 % 64 == 0 (64 ... 1024), Cout % 64 == 0, L >= 128, M % L == 0 (M need not be a multiple of
 * the 128-row block); pointers and row strides 16-byte multiples; h and x must not overlap Y (whole address ranges are compared).
 * Anything else is an argument error before any launch: no fallback inside the library. */
int mmd_res_tail(const void* h, int64_t ldh, const float* ga, const float* gb, int act, const void* W, const float* bias, const void* x,
                 int64_t ldx, const void* W2, const float* bias2, void* Y, int64_t ldy, int M, int L, int K1, int K2, int Cout,
                 float* stats, int64_t stats_ld, void* stream);

/* Spatial 3x3 conv whose input GroupNorm32(+FiLM)(+SiLU) is applied to the staged halo tile in LDS (tile 130, bf16, the nine
 * (0, dh, dw) taps, slices of whole frames): Y = conv3x3(act(A * gn_a[s(m)] + gn_b[s(m)])) + bias (+ R), zero padding of the
 * NORMALISED activation.  Replaces GroupNorm32 -> SiLU -> video_conv_spatial of the ResBlock in_layers (unet:339-340,83-99,
 * 457-458; nn.py:16-33) in one launch; bitwise equal to mmd_gn_apply followed by mmd_conv_gemm tile 130.  tile = 130 or 133. */
int mmd_gn_conv_gemm(int dtype, const void* A, int64_t lda, const float* gn_a, const float* gn_b, int act, int S,
                     int64_t rows_per_slice, const void* W, const float* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                     int M, int Cout, int Cin, int ntaps, const int* taps, int D0, int D1, int D2, int tile, void* stream);

/* VideoConv '2d+1d' in ONE launch (round 4): Y = conv1d_t(conv2d_s(act(X * gn_a[s] + gn_b[s]))) - the per-frame 3x3 conv, then the
 * per-pixel k=3 conv along the 16 frames (unet:83-99), with the ResBlock in_layers GroupNorm32 + SiLU applied to the staged input
 * (unet:339-340,457-458; nn.py:16-33; gn_a == NULL: plain conv) and, optionally, the statistics of Y for the out_layers norm
 * (quad records as mmd_conv_gemm_stats writes them; 4 records per block: record (n * H * W / 16 + patch) * 4 + frame group, i.e.
 * records are only meaningful to norms whose slices are whole samples).  bf16; X rows [N * 16 * H * W, Cin] (row stride ldx), Y rows
 * [.., 128]; F == 16, Cout == 128, Cin % 32 == 0, H % 4 == 0, W % 4 == 0; norm slices = whole samples.  The spatial result is rounded
 * to bf16 with its bias before the temporal conv (what a two-launch path stores); zero padding pads the NORMALISED activation.
 * Wf: the weight image of mmd_vconv2d1d_pack (mmd_vconv2d1d_weight_bytes(Cin) bytes) built from the packed spatial [128][9 * Cin]
 * and temporal [128][3 * 128] matrices (K index = tap * C + ci). */
int64_t mmd_vconv2d1d_weight_bytes(int Cin);
int mmd_vconv2d1d_pack(const void* Ws, const void* Wt, void* out, int Cin, int Cout, void* stream);
int mmd_vconv2d1d(const void* X, int64_t ldx, const float* gn_a, const float* gn_b, int act, int S, int64_t rows_per_slice,
                  const void* Wf, const float* bias_s, const float* bias_t, void* Y, int64_t ldy, int N, int F, int H, int W,
                  int Cin, int Cout, float* stats, int64_t stats_ld, void* stream);

/* The temporal-attention block of the video stream in ONE launch (round 4): Y = X + proj_out(attention over the 16 frames of each
 * pixel of qkv(GroupNorm32(X))) - SingleModalAtten with temporal sequences (unet:246-287 as used at :485-493: norm = nn.py:16-33 over
 * (16 frames, C / 32 channels) of a pixel, qkv / proj_out 1x1 convs, QKVAttention unet:290-330 with 1 / sqrt(ch) scaling).  Replaces
 * mmd_gn_small + mmd_conv_gemm (qkv) + mmd_attn_small_fwd + mmd_conv_gemm (proj_out, residual): the normalised tensor, the qkv tensor
 * and the attention output never exist in HBM (q, k, v and the attention output are rounded to bf16 exactly where the unfused path
 * stores them).  bf16; X / Y rows (n, f, pixel) x C with row strides ldx / ldy, Y != X; built for F == 16, heads == 4, C == 256
 * (head width 64: the ds2 level; the 384 / 512-channel instances of round 4 were removed in round 5), HW % 8 == 0.  Wf: the image of mmd_tattn_pack (mmd_tattn_weight_bytes(C, with_pre) bytes) built
 * from the qkv weight [3 C, C] (rows q | k | v, head h = rows h ch .. of each third) and the proj_out weight [C, C], both bf16
 * row-major.  bias_qkv [3 C], bias_proj / gamma / beta [C] fp32.  stats (nullable): quad statistics records of Y for the GroupNorm
 * that consumes it, one per 64 rows in THIS kernel's row order inside a sample (record n HW / 4 + (pixel >> 2): the 16 frames of 4
 * consecutive pixels), so only norms over whole samples may finalize from them.
 * Optional front stage (A != NULL, Wf packed with Wpre [C, C]): the block's input is x = X + A Wpre^T + bias_pre, i.e. the proj_out
 * 1x1 conv + residual of the SPATIAL attention block that precedes the temporal one (unet:485-490) rides in the same launch; MID
 * [rows, C] (distinct from X, A, Y) receives x, rounded to bf16 like the tensor the unfused path stores, and is re-read as operand
 * and as the residual of the last stage.  A == NULL: Wpre == NULL at pack time, MID / bias_pre unused. */
int64_t mmd_tattn_weight_bytes(int C, int with_pre);
int mmd_tattn_pack(const void* Wpre, const void* Wqkv, const void* Wproj, void* out, int C, void* stream);
int mmd_tattn_block(const void* X, int64_t ldx, const void* A, int64_t lda, void* MID, int64_t ldm, const void* Wf,
                    const float* bias_pre, const float* bias_qkv, const float* bias_proj, const float* gamma, const float* beta,
                    float eps, void* Y, int64_t ldy, int N, int F, int HW, int C, int heads, float* stats, int64_t stats_ld,
                    void* stream);

/* The temporal half of VideoConv '2d+1d' (unet:83-99: the per-pixel k = 3 conv along the frames, after the per-frame 3x3 conv) with
 * the activations stationary in registers (round 4): rows are gathered per pixel, the 16 frames of a pixel are the 16 lanes of a DPP
 * row, and the operand of tap df is the x fragment shifted by df lanes (zeros shifted in = the conv's zero padding in time), so every
 * activation row is loaded once instead of once per tap.  Bitwise equal to mmd_conv_gemm with the temporal taps.  bf16; X / Y rows
 * (n, f, pixel) x Cin / Cout (Y != X); F == 16, Cin in {256, 384, 512}, Cout % 64 == 0 (<= 512), HW % 8 == 0.  Wf: the image of
 * mmd_tconv_pack (mmd_tconv_weight_bytes(Cin, Cout) bytes) built from the packed GEMM matrix [Cout][3 * Cin] (K = tap * Cin + ci, taps
 * df = -1, 0, +1) that mmd_conv_gemm takes.  stats (nullable): quad statistics records of Y, one per 64 rows in THIS kernel's row
 * order inside a sample (record n HW / 4 + (pixel >> 2): the 16 frames of 4 consecutive pixels) - for norms over whole samples. */
int64_t mmd_tconv_weight_bytes(int Cin, int Cout);
int mmd_tconv_pack(const void* W, void* out, int Cin, int Cout, void* stream);
int mmd_tconv(const void* X, int64_t ldx, const void* Wf, const float* bias, void* Y, int64_t ldy, int N, int F, int HW, int Cin,
              int Cout, float* stats, int64_t stats_ld, void* stream);

/* The audio half of a ResBlock's in_layers in one launch (round 6): GroupNorm32(+FiLM) + SiLU + AudioConv (Conv1d, kernel 3, dilation,
 * zero "same" padding) on channels-last rows of S = M / L samples (unet:339-346, 108-131; nn.py:16-33) - instead of mmd_gn_apply followed
 * by mmd_conv_gemm with the taps (-d, 0, +d).  bf16.  X [M, ldx] (Cin columns), W [Cout][3 Cin] (mmd_conv_gemm's weight layout),
 * ga / gb [S, Cin] = the fused affine written by mmd_gn_finalize_stats / mmd_gn_stats, act != 0: SiLU; a tap that leaves its sample
 * contributes zero (the padding is zero AFTER the norm).  stats (nullable): quad records of Y as mmd_conv_gemm_stats writes them
 * (M % 64 == 0).  Bitwise equal to the two launches it replaces (same K order, same rounding points). */
int mmd_aconv(const void* X, int64_t ldx, const void* W, const float* bias, const float* ga, const float* gb, int act, void* Y, int64_t ldy,
              int M, int L, int Cin, int Cout, int dil, float* stats, int64_t stats_ld, void* stream);

/* softmax(q k^T / sqrt(ch)) v over query groups with circular key windows - SingleModalQKVAttention
 * (unet:221-240) and the random-shift cross-modal QKVAttention (unet:507-564; window addressing unet:614-647).
 * For batch n, group g (< G): queries = Q rows n*q_rows_per_batch + g*q_per_group + [0, q_per_group) (the last
 * group extends to q_rows_per_batch); keys = KV rows n*k_rows_per_batch + ((g + shift)*k_per_group + j) mod
 * k_rows_per_batch, j < win*k_per_group.  shift_dev: device int (nullable = 0) so a captured graph can be
 * replayed with a new shift.  Head h uses columns {q,k,v}_off + h*ch.  impl: 0 auto, 1 force the VALU kernel, 2 the per-128-query
 * MFMA kernel (register-staged K / V), 3 the staged-window kernel, 4 the DMA-staged kernel (head width 64: K / V tiles by
 * buffer_load ... lds, V^T fragments by transposing LDS reads; bitwise equal to 2), 5 the software-pipelined kernel whose loop
 * iteration is one hand-written instruction stream (head width 64; bitwise equal to 2). */
int mmd_attn_fwd(int dtype, const void* Q, int64_t ldq, int q_off, const void* KV, int64_t ldkv, int k_off, int v_off, void* O,
                 int64_t ldo, int heads, int ch, int nb, int G, int64_t q_rows_per_batch, int q_per_group,
                 int64_t k_rows_per_batch, int k_per_group, int win, const int* shift_dev, int impl, void* stream);
/* Self-attention over short strided slices (temporal attention '(b h w) c f', unet:489-490): rows hold
 * [q(C)|k(C)|v(C)]; slice geometry as mmd_gn_stats; Tn <= 32. */
int mmd_attn_small_fwd(int dtype, const void* QKV, int64_t ld, void* O, int64_t ldo, int C, int heads, int S, int Tn, int inner,
                       int64_t outer_stride, int64_t inner_stride, int64_t tstride, void* stream);

/* Downsample (avg-pool, mode 0) / Upsample (nearest, mode 1) by (1, fh, fw) on rows (nf, h, w)
 * (unet:133-208: video (1,2,2); audio F=1,H=1,W=L, fw=4).  H, W describe the INPUT. */
int mmd_resample(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int C, int NF, int H, int W, int fh, int fw,
                 int mode, float scale, void* stream);   /* y = scale * resample(x): backward of one mode is the other mode, rescaled */
/* The same resampling (bf16, scale 1) with the GroupNorm statistics of the OUTPUT in the epilogue: stats / stats_ld as in
 * mmd_conv_gemm_stats - one (sum, sum of squares) record per 64 output rows and QUAD of channels, of the values as stored.  The norms
 * that follow a resample (the out_layers norm of a down ResBlock, every norm over an up ResBlock's output: unet:441-448 + nn.py:16-33)
 * then finalize with mmd_gn_finalize_stats instead of a statistics pass.  Output rows % 64 == 0, C % 8 == 0, C <= 2048. */
int mmd_resample_stats(const void* x, int64_t ldx, void* y, int64_t ldy, int C, int NF, int H, int W, int fh, int fw, int mode,
                       float* stats, int64_t stats_ld, void* stream);
/* 2-D strided copy (skip-connection concat th.cat, unet:1093-1094). */
int mmd_copy2d(const void* x, int64_t ldx_bytes, void* y, int64_t ldy_bytes, int64_t rows, int64_t row_bytes, void* stream);

/* Stem: API layout fp32 x[N,F,Cin,H,W] (audio F=1,H=1,W=L) -> channels-last rows; W fp32 [ntaps][Cin][Cout]
 * (InitialBlock, unet:680-694: spatial 3x3 half of the 2d+1d conv, and the audio k=3 conv). */
int mmd_stem_conv(int dtype, const float* x, const float* w, const float* bias, void* y, int64_t ldy, int N, int F, int Cin,
                  int H, int W, int Cout, int ntaps, const int* taps, void* stream);
/* Head: channels-last rows (after GN+SiLU) -> API layout fp32 y[N,F,Co,H,W]; W fp32 [ntaps][Cin][Co], Co <= 8
 * (video_out Conv3d 3x3x3 / audio_out Conv1d k3, unet:1003-1012). */
int mmd_head_conv(int dtype, const void* x, int64_t ldx, const float* w, const float* bias, float* y, int N, int F, int Cin,
                  int H, int W, int Co, int ntaps, const int* taps, void* stream);
/* The same head for few output channels as GEMM + gather (round 5; bf16, Cin = 128, ntaps * Co <= 96): mmd_head_gemm computes the
 * per-row products P[tap Co + co][m] = sum_ci W[tap][ci][co] act(x[m][ci] a + b) on the matrix cores - the GroupNorm32 + SiLU of
 * video_out.0/.1 (unet:1003-1006) applied in registers from the fused affine a / b [S, Cin] (S slices of gn_rows rows, gn_rows % 128
 * == 0), x read once, nothing normalised written - and mmd_head_gather sums them over the taps into the API layout
 * y[N, F, Co, H, W] (+ bias; zero padding outside (F, H, W)).  wimg: the bf16 (hi, lo) weight image in MFMA fragment order,
 * mmd_head_gemm_weight_bytes(Cin) bytes, packed by the host mirror (ops.head_gemm_pack); P: fp32 workspace [ntaps * Co][M]. */
int64_t mmd_head_gemm_weight_bytes(int Cin);
int64_t mmd_head_gemm_workspace_bytes(int64_t M, int ntaps, int Co);
int mmd_head_gemm(const void* x, int64_t ldx, int64_t M, int Cin, const float* gn_a, const float* gn_b, int S, int64_t gn_rows, int act,
                  const void* wimg, float* P, int NO, void* stream);
int mmd_head_gather(const float* P, const float* bias, float* y, int N, int F, int H, int W, int Co, int ntaps, const int* taps,
                    void* stream);

/* One DDPM ancestral step for one stream (p_mean_variance + p_sample, multimodal_gaussian_diffusion.py:231-343,
 * 415-474) on API-layout fp32 tensors x/noise/out [N,F,C,HW], model_out [N,F,Cm,HW] (Cm = 2C with flag 4).
 * tables fp32 [7][T]: sqrt_recip_ac, sqrt_recipm1_ac, post_c1, post_c2, fixed logvar, min_log, max_log;
 * t int64[N] device.  flags: 1 clip x0, 2 model predicts x0, 4 learned-range variance.  out (sample = mean +
 * [t!=0] exp(logvar/2) noise), x0_out, mean_out, logvar_out are each nullable (p_mean_variance alone: out = NULL). */
int mmd_ddpm_update(const float* x, const float* model_out, const float* noise, float* out, float* x0_out, float* mean_out,
                    float* logvar_out, const float* tables, const int64_t* t, int T, int N, int F, int C, int HW, int flags,
                    void* stream);
/* q_sample (gd:187-205): out = tab2[0][t] x0 + tab2[1][t] eps. */
int mmd_q_sample(const float* x0, const float* eps, float* out, const float* tab2, const int64_t* t, int T, int N,
                 int64_t per_sample, void* stream);

/* Per-sample loss terms of multimodal_training_losses for one stream (gd:1114-1203; vb term _vb_terms_bpd gd:1048-1092,
 * losses.py:12-77): mse_out[n] = mean((target - eps_hat)^2); with flag 4 also vb_out[n] (KL for t>0, decoder NLL at t==0,
 * in bits, frozen mean, clip off) * vb_scale.  Layouts as mmd_ddpm_update; deterministic two-stage reduction. */
int64_t mmd_loss_workspace_bytes(int N);
int mmd_loss_terms(const float* x0, const float* xt, const float* model_out, const float* target, const float* tables,
                   const int64_t* t, int T, int N, int F, int C, int HW, int flags, float vb_scale, float* mse_out, float* vb_out,
                   void* workspace, void* stream);

/* One term of the variational bound in bits / dim for one stream (_vb_terms_bpd + the per-step reductions of calc_bpd_loop, gd:1048-1092,
 * 1231-1286), one pass: vb (KL for t>0, decoder NLL at t==0, model mean live), xstart_mse = mean((pred_x0 - x0)^2), eps_mse =
 * mean((eps(pred_x0) - noise)^2).  flags 1 / 2 / 4 as mmd_ddpm_update (fixed variance: model log-variance = table row 4; the true
 * posterior's is row 5).  Results of sample n go to column t[n] of row n of the fp32 tables [N, out_ld] (out_ld == 0: fp32 [N]), so a
 * whole loop runs from a captured graph and is read back once.  noise / xstart_mse_out / eps_mse_out / pred_xstart_out are nullable.
 * Deterministic fixed-order reduction.  The per-element arithmetic is the device function of mmd_loss_terms instantiated in double: with
 * flag 4 and clip off vb agrees with mmd_loss_terms' vb (vb_scale 1) to the accuracy of that fp32 evaluation. */
int64_t mmd_vlb_workspace_bytes(int N);
int mmd_vlb_terms(const float* x0, const float* xt, const float* noise, const float* model_out, const float* tables, const int64_t* t,
                  int T, int N, int F, int C, int HW, int flags, float* vb_out, float* xstart_mse_out, float* eps_mse_out,
                  int64_t out_ld, float* pred_xstart_out, void* workspace, void* stream);
/* Gradient of sum_n dvb[n] vb[n] of mmd_vlb_terms w.r.t. the model output (KL / RESCALED_KL training, gaussian_diffusion.py:872-882): the
 * mean channels get the KL / NLL gradient through pred_x0 -> posterior mean, the variance channels as mmd_loss_terms_bwd.  Clip off only. */
int mmd_vlb_terms_bwd(const float* x0, const float* xt, const float* model_out, const float* tables, const int64_t* t, int T, int N,
                      int F, int C, int HW, int flags, const float* dvb, float* g_model_out, void* stream);

/* ---------------------------------------------------------------- training step: backward kernels (gd:1114-1203 backward)
 * conv wgrad: dW fp32 [Cout][ntaps*Cin] += dY^T gather(X) (same tap semantics as mmd_conv_gemm; caller zeroes dW), db
 * (nullable, fp32 [Cout]) += column sums of dY.  conv dgrad = mmd_conv_gemm(dY, W^T-packed, taps negated).  bf16 with >= 64 channels on
 * both sides: 128 x 128 MFMA tiles split over M with fp32 atomics (the accumulation order - and the last bit - varies from run to run,
 * like the reference's autograd); 9-tap convs stage row-major by descriptor DMA and read both operands with transposing LDS reads. */
int mmd_conv_wgrad(int dtype, const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, float* db, int M, int Cout, int Cin,
                   int ntaps, const int* taps, int D0, int D1, int D2, int torch_layout, void* stream);
/* Re-pack every conv weight in ONE launch after an optimizer step.  descs_dev: device array of n records
 *   { const float* src; void* fwd; void* bwd; int Cout, Cin, nt; int block_start; }   (block_start = running sum of mmd_pack_blocks(Cout, Cin, nt):
 *   one workgroup per tile of 32 output x (216 / nt) input channels x all taps, staged through LDS so that both operands are written in runs; nt <= 27)
 * src fp32 [Cout][Cin][nt] (torch conv layout) -> fwd [Cout][nt*Cin] (mmd_conv_gemm operand of the forward conv) and
 * bwd [Cin][nt*Cout] (operand of the data-gradient conv), both in `dtype`.  mmd_conv_wgrad with torch_layout = 1 accumulates
 * dW directly in [Cout][Cin][nt], i.e. straight into the parameter's .grad. */
int mmd_pack_blocks(int Cout, int Cin, int nt);     /* workgroups of one record (-1: unsupported tap count) */
int mmd_pack_conv_weights(int dtype, const void* descs_dev, int n, int total_blocks, void* stream);
/* Gradient counterpart, once per step: for every record (same struct; src = the parameter's fp32 .grad [Cout][Cin][nt], fwd = an
 * fp32 packed accumulation buffer [Cout][nt*Cin] that mmd_conv_wgrad filled with coalesced atomics) grad += packed, packed = 0. */
int mmd_unpack_conv_grads(const void* descs_dev, int n, int total_blocks, void* stream);
/* GroupNorm32(+FiLM)(+SiLU) backward; a, b, mr from the forward mmd_gn_stats; dgamma/dbeta accumulate; dfilm (nullable)
 * [S, >=2C] receives (dscale | dshift); workspace (S*C*2 + S*64) floats.  C a multiple of 32 and of the 16-byte vector, C <= 2048
 * (the forward's limit; launch shapes for C <= 1024 are what they always were, fp32 rows above 1024 channels go in two column
 * halves), S <= 65535. */
int mmd_gn_bwd(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int64_t rows, int C, int S,
               int Tn, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tstride, const float* a, const float* b,
               const float* mr, const float* gamma, const float* beta, const float* film, int64_t film_ld, int act, float* dgamma,
               float* dbeta, float* dfilm, int64_t dfilm_ld, float* workspace, void* stream);
/* The same with a CALLER-KEPT workspace whose first S*C*2 floats are zero on entry; they are zero again on exit (the parameter stage
 * clears what it read), so the fill launch in front of every norm's backward is gone (243 per training step, mtu:280-330).  One
 * workspace per stream and per value of S*C; zero it once after allocation.  The group means are left behind the accumulators, at
 * workspace + S*C*2: a kept workspace may be reused only for calls with the same S*C (a call with another S*C and the same total
 * length S*(2C+64) would accumulate onto those means). */
int mmd_gn_bwd_ws0(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int64_t rows, int C, int S,
                   int Tn, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tstride, const float* a, const float* b,
                   const float* mr, const float* gamma, const float* beta, const float* film, int64_t film_ld, int act, float* dgamma,
                   float* dbeta, float* dfilm, int64_t dfilm_ld, float* workspace, void* stream);
/* Attention backward for every attention of the model (strided + windowed row descriptor, see mmd_attn_bwd.hip).  Head width
 * ch <= 192: 64-row LDS tiles up to 128, 32-row tiles above (the fp32 path and the bf16 path of widths off the MFMA list). */
int mmd_attn_bwd(int dtype, const void* Q, int64_t ldq, int q_off, const void* KV, int64_t ldkv, int k_off, int v_off, const void* O,
                 int64_t ldo, const void* dO, int64_t lddo, void* dQ, int64_t lddq, int dq_off, void* dKV, int64_t lddkv, int dk_off,
                 int dv_off, float* lse_ws, float* dsum_ws, int heads, int ch, int nb, int G, int q_inner, int64_t q_outer,
                 int64_t q_istride, int64_t q_tstride, int q_total, int q_per_group, int k_inner, int64_t k_outer, int64_t k_istride,
                 int64_t k_tstride, int k_mod, int k_per_group, int win, const int* shift_dev, void* stream);
/* bf16 MFMA pair for contiguous-row attention: the training forward also returns the log2-domain log-sum-exp per (query
 * row, head); the backward recomputes P from it (no stored probabilities).  Same row / window arguments as mmd_attn_fwd.
 * Head widths {16,32,48,64,96,128,192}; at 192 the dK / dV kernel runs as two workgroups per (key tile, head), each accumulating
 * 96 of the 192 columns (the one-workgroup form needs 352 live registers and spills). */
int mmd_attn_fwd_lse(int dtype, const void* Q, int64_t ldq, int q_off, const void* KV, int64_t ldkv, int k_off, int v_off, void* O,
                     int64_t ldo, int heads, int ch, int nb, int G, int64_t q_rows_per_batch, int q_per_group,
                     int64_t k_rows_per_batch, int k_per_group, int win, const int* shift_dev, float* lse2_out, void* stream);
int mmd_attn_bwd_mfma(const void* Q, int64_t ldq, int q_off, const void* KV, int64_t ldkv, int k_off, int v_off, const void* O,
                      int64_t ldo, const void* dO, int64_t lddo, void* dQ, int64_t lddq, int dq_off, void* dKV, int64_t lddkv,
                      int dk_off, int dv_off, const float* lse2, float* dsum_ws, int heads, int ch, int nb, int G,
                      int64_t q_rows_per_batch, int q_per_group, int64_t k_rows_per_batch, int k_per_group, int win,
                      const int* shift_dev, void* stream);
/* DDIM step for one stream (ddim_sample gd:821-901; flag 8 = ddim_reverse_sample gd:903-953).  tables as mmd_ddpm_update,
 * tab3 [3,T] fp32 = alphas_cumprod, alphas_cumprod_prev, alphas_cumprod_next; flags 1 clip, 2 model predicts x0, 4 learned sigma. */
int mmd_ddim_update(const float* x, const float* model_out, const float* noise, float* out, float* x0_out, const float* tables,
                    const float* tab3, const int64_t* t, int T, int N, int F, int C, int HW, int flags, float eta, void* stream);
/* Counter-based noise: N(0,1) values that are a pure function of (seed, sample id, draw, stream tag, element), so a sample does not
 * depend on its batch position, the batch size, the lane or the rank.  Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 /
 * 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85), key = the 64-bit seed, low word first (key: device, 2 words), counter
 *   c0 = r >> 2   r = the element's index inside its sample in API layout ([F,C,H,W] video, [C,L] audio, [C,H,W] SR image)
 *   c1 = draw     the loop index t[n] the update kernels read (SpacedDiffusion: the respaced index); 0xFFFFFFFF = x_T; the resampled
 *                 masked loop hands its draws in (mmd_ddpm_update_ctr_at, mmd_renoise_ctr): i + r T for visit r of step i, 0x80000000 + k
 *                 for the k-th forward jump; the stochastic solver step (mmd_dpmpp_sde_update_ctr) draws at the evaluation number k[n], the
 *                 table row it reads anyway (below 2^31, like the loop indices)
 *   c2 = sample id  ids[n] (device int64 [N]); the low 32 bits are used and the HOST refuses ids outside [0, 2^32) (mm_diffusion/seeded.py:
 *                 the library cannot look into device memory without a sync)
 *   c3 = tag      0 video, 1 audio, 2 SR image, 3 window shifts (host only)
 * The four output words belong to elements 4 c0 ... 4 c0 + 3 (one Philox evaluation per four outputs); words past the end of a sample
 * are dropped.  Word w -> u = ((w >> 9) + 0.5) 2^-23 (exact in fp32, inside (0, 1)); words 0, 1 -> z0 = rho cos(2 pi u1), z1 = rho
 * sin(2 pi u1), rho = sqrt(-2 ln u0), words 2, 3 likewise -> z2, z3: precise logf / sqrtf and sincospif(2 u), no fast intrinsics.
 * The largest |z| is sqrt(2 * 24 ln 2) = 5.77.  Seed and ids live in device memory so that a captured graph does not bake them in.
 * mmd_ctr_fill: out [N, per_sample], kind 0 = the fp32 normals, kind 1 = the raw uint32 words (tests, diagnosis); it serves x_T, the
 * fixed conditioning noise of the replacement loop and the eager noise_source(like) call.  No LDS, no library state. */
int mmd_ctr_fill(void* out, int kind, const uint32_t* key, const int64_t* ids, int N, int64_t per_sample, uint32_t draw, int tag,
                 void* stream);
/* mmd_ddpm_update / mmd_ddim_update with the noise drawn in the kernel from the counter above (draw = t[n]) instead of read from
 * memory: bitwise the memory form fed with mmd_ctr_fill(kind 0) of the same key, ids, tag and draw.  A thread owns one quad of
 * consecutive elements of a sample. */
int mmd_ddpm_update_ctr(const float* x, const float* model_out, const uint32_t* key, const int64_t* ids, int tag, float* out, float* x0_out,
                        float* mean_out, float* logvar_out, const float* tables, const int64_t* t, int T, int N, int F, int C, int HW,
                        int flags, void* stream);
int mmd_ddim_update_ctr(const float* x, const float* model_out, const uint32_t* key, const int64_t* ids, int tag, float* out, float* x0_out,
                        const float* tables, const float* tab3, const int64_t* t, int T, int N, int F, int C, int HW, int flags, float eta,
                        void* stream);
/* mmd_ddpm_update_ctr with counter word c1 = the low 32 bits of draw[n] (device int64 [N]) instead of t[n]: a loop that runs a timestep
 * more than once (the resampling jumps of masked sampling) gives every visit noise of its own.  Bitwise the memory form fed with
 * mmd_ctr_fill(draw); with draw == t bitwise mmd_ddpm_update_ctr.  Draw convention of the resampled loop (mm_diffusion/masking.py,
 * repaint_schedule): visit r = 0, 1, ... of step i of T draws i + r T (below 2^31, so the first visit draws what the plain loop draws),
 * the k-th forward jump draws 0x80000000 + k, and 0xFFFFFFFF stays x_T. */
int mmd_ddpm_update_ctr_at(const float* x, const float* model_out, const uint32_t* key, const int64_t* ids, int tag, float* out, float* x0_out,
                           float* mean_out, float* logvar_out, const float* tables, const int64_t* t, const int64_t* draw, int T, int N,
                           int F, int C, int HW, int flags, void* stream);
/* The forward jump of resampled masked sampling (RePaint, Lugmayr et al., CVPR 2022), in place on x fp32 [N, F, C, HW]: x = a x + b z
 * with a = jtab[m[n]], b = jtab[T + m[n]] and z = the counter normal of (element, draw[n], ids[n], tag).  jtab fp32 [2, T]: a[m] =
 * sqrt(ac[m + J] / ac[m]), b[m] = sqrt(1 - ac[m + J] / ac[m]) for a jump of J levels (the host computes them in float64; entries with
 * m + J > T - 1 are zero and never used).  The element is mmd_q_sample's, so the result is bitwise mmd_ctr_fill(draw) followed by
 * mmd_q_sample(x, eps, x, jtab, m) - which is also the memory form of the jump.  One quad per thread; an m[n] outside [0, T) writes
 * nothing. */
int mmd_renoise_ctr(float* x, const uint32_t* key, const int64_t* ids, int tag, const float* jtab, const int64_t* m, const int64_t* draw,
                    int T, int N, int F, int C, int HW, void* stream);
/* Masked conditioning of the replacement method (gd:642-720 overwrites a whole stream with q_sample(condition, t, noise = that stream's
 * x_T) before every step; here any part of it): in place, x = A known + B eps where the mask cell is set; elsewhere x is NOT written.
 * x / known / noise fp32 [N, F, C, HW] (audio: F = 1, HW = L).  mask uint8, one cell per (frame, position) shared by the channels: element
 * (n, f, c, p) reads mask[n * mask_stride + f * HW + p]; mask_stride = 0 (one mask for the batch) or F * HW (one per sample); non-zero =
 * known; mask == NULL = the whole stream.  A, B = tab2[t[n]], tab2[T + t[n]] (mmd_q_sample's table; a t[n] outside [0, T) replaces
 * nothing), or the host scalars ca, cb with t == NULL.  On known cells the result is bitwise what mmd_q_sample writes.  eps = noise[i], or
 * (_ctr) the counter normal of (element, draw 0xFFFFFFFF, ids[n], tag): the value mmd_ctr_fill gives the element at the x_T draw, so no
 * buffer holds the fixed conditioning noise.  noise may be NULL with t == NULL and cb == 0 only: x = ca known (ca = 1: the final paste,
 * bitwise `known`). */
int mmd_cond_replace(float* x, const float* known, const float* noise, const uint8_t* mask, int64_t mask_stride, const float* tab2,
                     const int64_t* t, float ca, float cb, int T, int N, int F, int C, int HW, void* stream);
int mmd_cond_replace_ctr(float* x, const float* known, const uint32_t* key, const int64_t* ids, int tag, const uint8_t* mask,
                         int64_t mask_stride, const float* tab2, const int64_t* t, float ca, float cb, int T, int N, int F, int C, int HW,
                         void* stream);
/* out[n,:] = (ca[t_n] a + cb[t_n] b) cs[t_n]: the _predict_* / q_posterior helpers (gd:170-229,345-366); NULL table = 1, b nullable. */
int mmd_lincomb_t(const float* a, const float* b, float* out, const float* ca, const float* cb, const float* cs, const int64_t* t,
                  int N, int64_t per_sample, void* stream);
/* out = ca a + cb b + cc c (b, c nullable): solver update combinations (multimodal_dpm_solver_plus.py:520-1100). */
int mmd_lincomb(const float* a, float ca, const float* b, float cb, const float* c, float cc, float* out, int64_t n, void* stream);
/* y = (dst dtype)(x * scale), fp32 <-> bf16: the bf16 payload of the data-parallel gradient all-reduce (reference: DDP reduces
 * the fp32 / fp16 gradients it is given, multimodal_train_util.py:127-136) and its widening + 1/world scaling afterwards. */
int mmd_cast(const void* x, int src_dtype, void* y, int dst_dtype, float scale, int64_t n, void* stream);
/* backward of mmd_ddpm_update's sample w.r.t. x and the model output (gradient-guided sampling gd:722-817; fixed variance). */
int mmd_ddpm_update_bwd(const float* x, const float* model_out, const float* dsample, float* dx, float* dmodel_out, const float* tables,
                        const int64_t* t, int T, int N, int64_t per_sample, int flags, void* stream);
/* DPM-Solver++ dynamic thresholding (multimodal_dpm_solver_plus.py:419-440): out[n] = q-quantile of |x[n,:]| (torch.quantile,
 * linear interpolation), exact radix select; then x[n,:] = clamp(x, -s, s) / (s / max_val) with s = max(s_n, 1), in place. */
int mmd_abs_quantile(const float* x, int N, int64_t per_sample, float q, float* out, void* stream);
int mmd_clamp_scale(float* x, const float* s, float max_val, int N, int64_t per_sample, void* stream);
/* One evaluation of the fixed-grid multistep DPM-Solver / DPM-Solver++ loop (multimodal_dpm_solver_plus.py:1252-1283) with every
 * coefficient in a device table, so that a captured step bakes in no scalar.  tab: fp32 [6][rows] = cx, ce, c0, c1, c2, kind; k: device
 * int64 [N], the step number (a sample whose k is outside [0, rows) is not written).  x / x0raw / M1: fp32 [N,F,C,HW]; the model output
 * fp32 [N,F,Cm,HW] with Cm = C or 2C, eps = its first C channels.
 *   mmd_dpmpp_x0      x0raw = cx[k] x + ce[k] eps: data_prediction_fn before its thresholding (dpm:419-428), mmd_lincomb's bits.  hist:
 *                     NULL, or the workspace below - the same pass then adds level 0 (top 11 magnitude bits) of |x0raw| to it.
 *   mmd_dpmpp_select  out[n] = q-quantile of |x[n,:]|, torch.quantile 'linear' (dpm:432,436): exact three-level (11 + 10 + 10 bits)
 *                     multi-workgroup selection of the two neighbouring ranks, bitwise what mmd_abs_quantile returns.  level0_done != 0:
 *                     mmd_dpmpp_x0 has filled level 0.  The workspace (mmd_dpmpp_workspace_bytes(N), per call in flight) must be zero
 *                     on entry and is zero again afterwards.  x must hold no NaN.
 *   mmd_dpmpp_update  m0 = clamp(m0, -s, s) / (s / max_val), s = max(s[n], 1) (dpm:433-434,437-438; s == NULL: m0 as it is), then by the
 *                     row's kind, in place: 0  x = c0 x + c1 m0 (dpm_solver_first_update, dpm:532-590; M1 is not read)
 *                     1  x = c0 x + c1 m0 + c2 M1 (multistep_dpm_solver_second_update, dpm:889-947)   2  x = m0 (denoise_fn, dpm:526-530);
 *                     and M1 = m0, the history of the next step.  m0: x0raw (Cm = C) or, for the noise-prediction solver, the model output.
 */
int64_t mmd_dpmpp_workspace_bytes(int N);
int mmd_dpmpp_x0(const float* x, const float* model_out, float* x0raw, const float* tab, const int64_t* k, int rows, void* hist, int N, int F,
                 int C, int Cm, int HW, void* stream);
int mmd_dpmpp_select(const float* x, void* workspace, int level0_done, int N, int64_t per_sample, float q, float* out, void* stream);
int mmd_dpmpp_update(float* x, const float* m0, float* M1, const float* s, float max_val, const float* tab, const int64_t* k, int rows, int N,
                     int F, int C, int Cm, int HW, void* stream);
/* One evaluation of the stochastic multistep solver in its data-prediction form (SDE-DPM-Solver++, Lu et al. 2022, "DPM++ 2M SDE" in
 * other toolkits; orders 1 and 2): mmd_dpmpp_update with a noise term.  tab, k, rows, the kinds and the geometry are mmd_dpmpp_update's
 * (tab fp32 [6][rows], layout unchanged); cz: fp32 [rows], the noise coefficient of each row.  With h = lambda_t - lambda_s > 0 and
 * E = -expm1(-2 h) the host fills c0 = (sigma_t / sigma_s) e^-h, c1 + c2 = alpha_t E (second order: c1 = alpha_t E (1 + 1 / (2 r0)),
 * c2 = -alpha_t E / (2 r0)), cz = sigma_t sqrt(E), so that c0 alpha_s + c1 + c2 = alpha_t and c0^2 sigma_s^2 + cz^2 = sigma_t^2: a
 * perfect data prediction keeps the marginal N(alpha_t mu, sigma_t^2) at any step size.  In place, by the row's kind:
 *   0  x = c0 x + c1 m0 + cz z (M1 is not read)     1  x = c0 x + c1 m0 + c2 M1 + cz z     2  x = m0 (no noise is read, no Philox evaluated)
 * and M1 = m0; m0 is clamp-scaled by s[n] first when s != NULL.  The sums are mmd_lincomb's, term by term in that order (one rounded
 * product, then one fma per further term, the noise last): bitwise mmd_clamp_scale + mmd_lincomb(x, c0, m0, c1, M1, c2) +
 * mmd_lincomb(v, 1, z, cz).  A sample whose k is outside [0, rows) writes nothing: not x, not M1.
 *   mmd_dpmpp_sde_update      z = noise[i], fp32 [N,F,C,HW].  x, M1 and noise must not overlap (checked).
 *   mmd_dpmpp_sde_update_ctr  z = the counter normal above with c1 (draw) = the low 32 bits of k[n], c2 = ids[n], c3 = tag, c0 = the
 *                             element's index inside its sample >> 2: bitwise mmd_ctr_fill(draw = k) followed by the memory form, and
 *                             no noise buffer exists.
 * A thread owns one quad of consecutive elements of a sample in both forms: 16-byte loads and stores where the quad is whole and its
 * address a multiple of 16, element by element otherwise (a ragged last quad; words past the end of a sample are dropped).  No LDS, no
 * library state. */
int mmd_dpmpp_sde_update(float* x, const float* m0, float* M1, const float* noise, const float* s, float max_val, const float* tab,
                         const float* cz, const int64_t* k, int rows, int N, int F, int C, int Cm, int HW, void* stream);
int mmd_dpmpp_sde_update_ctr(float* x, const float* m0, float* M1, const uint32_t* key, const int64_t* ids, int tag, const float* s,
                             float max_val, const float* tab, const float* cz, const int64_t* k, int rows, int N, int F, int C, int Cm,
                             int HW, void* stream);
/* Spherical interpolation of two latents, row by row: a, b, out fp32 [N, per], lam fp32 [N] (device), out[n] = w_a a[n] + w_b b[n] with
 *   dot = sum a b, na = sum a^2, nb = sum b^2      fp64 sums of the fp32 data (every product is exact in fp64)
 *   c = clamp(dot / sqrt(na nb), -1, 1), theta = acos c, s = sin theta
 *   w_a = sin((1 - lam) theta) / s, w_b = sin(lam theta) / s;      na nb == 0 or |c| > 0.9995: w_a = 1 - lam, w_b = lam (the chord)
 * The weights are formed in fp64 by one thread and rounded to fp32 once; the combine is fma(w_a, a, fl(w_b b)), so the error of out is
 * two weight roundings, one product rounding and one fused add.  lam = 0 / 1 gives weights exactly (1, 0) / (0, 1): out is bitwise a / b
 * for finite data without negative zeros.  lam outside [0, 1] extrapolates.
 * Two launches over a grid of (chunks of a sample, N): partial sums into ws (fp64 [N, chunks, 3], mmd_slerp_ws_bytes(N, per) bytes, host
 * only, 0 for bad arguments), then the combine, whose every workgroup re-reduces the chunks of its sample in one fixed tree order.  No
 * atomics, no host read, no library state: legal inside a stream capture.  The chunking depends on per alone and the order of every sum
 * on the element index alone, so row n is bitwise the same in any batch and at any buffer address.  16-byte loads and stores where a quad
 * of consecutive elements is whole and its address a multiple of 16 (a, b and out each by their own address), element by element
 * otherwise.  Refused before anything is launched: a NULL pointer, N <= 0 (or > 65535), per <= 0, out overlapping a or b (a and b may
 * overlap: slerp(a, a) = a by the chord). */
int64_t mmd_slerp_ws_bytes(int N, int64_t per);
int mmd_slerp(const float* a, const float* b, const float* lam, float* out, double* ws, int N, int64_t per, void* stream);
/* One evaluation of the single-step DPM-Solver / DPM-Solver++ loop (multimodal_dpm_solver_plus.py:1277-1294; orders 1-3, dpm:532-887)
 * from the same kind of table (fp32 [6][rows] = cx, ce, c0, c1, c2, kind; k as above; a sample whose k is outside [0, rows) writes
 * nothing: not x, not XB, not MS).  A step of order p is p evaluations; its later stages combine the state and the model value at the
 * step's START with the newest model value, so the step keeps two histories, both fp32 [N,F,C,HW]: XB, the state there, and MS, the
 * model value there.  XB and MS must overlap neither x nor each other (x is updated in place; checked).
 *   m0     form 0: the first C of src's Cm channels (src fp32 [N,F,Cm,HW], Cm = C or 2C: the model output for the noise-prediction
 *          solver, or the x0raw that mmd_dpmpp_x0 filled, Cm = C), then clamp(m0, -s, s) / (s / max_val), s = max(s[n], 1), when s != NULL
 *          form 1: cx[k] x + ce[k] eps, eps = the first C channels of src (the data prediction without thresholding, the bits of
 *          mmd_dpmpp_x0 followed by form 0 without that launch); s must be NULL
 *   kind   0 open, the first evaluation of a step of any order: XB = x, MS = m0, x = c0 x + c1 m0
 *          1 stage, the second or third evaluation: x = c0 XB + c1 MS + c2 m0; XB and MS are not written
 *          2 denoise (denoise_fn, dpm:526-530): x = m0; XB and MS are not written
 * The sums are mmd_lincomb's, term by term (one product, then one fma per further term). */
int mmd_dpm_single_update(float* x, const float* src, int form, float* XB, float* MS, const float* s, float max_val, const float* tab,
                          const int64_t* k, int rows, int N, int F, int C, int Cm, int HW, void* stream);
/* adaptive-step error term (dpm:1088-1149): out[n] += sum(((hi - lo) / max(atol, rtol max(|lo|, |prev|)))^2), fp64, caller zeroes. */
int mmd_dpm_err(const float* hi, const float* lo, const float* prev, float atol, float rtol, int N, int64_t per_sample, double* out,
                void* stream);
/* --- the adaptive DPM-Solver++ of order 2 with its step-size controller on the device (DPM_Solver.sample_graph_adaptive; the eager
 * loop, multimodal_dpm_solver_plus.py dpm_solver_adaptive, reads one scalar back per trial step).  A trial step s -> t = lambda^-1(lambda_s
 * + h) evaluates the network at (x, s) and at (x_s1, s1 = lambda^-1(lambda_s + h / 2)).  Data prediction only.  All four kernels are
 * ordinary launches without atomics or library state, legal inside a stream capture; arguments are refused before anything is launched
 * (a NULL pointer, N <= 0, overlapping buffers).  x / XB / MS / LO / PREV: fp32 [N,F,C,HW]; src fp32 [N,F,Cm,HW], Cm = C or 2C; tab: fp32
 * [6][rows] and k: int64 [N] as in mmd_dpm_single_update (a sample whose k is outside [0, rows) writes nothing) - the stepper uses
 * rows = N and k[n] = n, the controller's per-sample rows, and k[n] = -1 once sample n is done.  m (the model value): form 0 / form 1 and
 * s / max_val exactly as in mmd_dpm_single_update, with tab rows 0, 1 = cx, ce.  The elementwise kernels own one quad per thread
 * (16-byte accesses where the quad is whole and aligned, element by element otherwise) and their sums are mmd_lincomb's term by term,
 * so they write the bits of the mmd_clamp_scale / mmd_lincomb / copy launches they replace.
 *   mmd_dpm_adapt_open     tab rows 2-5 = a0, a1, b0, b1.  XB = x, MS = m0, LO = a0 x + a1 m0 (the first-order result at t),
 *                          x = b0 x + b1 m0 (the first-order result at s1: the next evaluation's input).
 *   mmd_dpm_adapt_close    tab rows 2-4 = c0, c1, c2.  x = c0 XB + c1 MS + c2 m1 (the second-order result at t, over x_s1), and in the
 *                          same pass the element term e = (x - LO) / max(atol, rtol max(|LO|, |PREV|)) in fp32 - mmd_dpm_err's
 *                          expression, atol and rtol read from params and rounded to fp32 - summed as e^2 in fp64 over a grid of
 *                          (chunks of a sample, N) into partial[n][chunk], chunks = mmd_dpm_adapt_chunks(F C HW) of
 *                          MMD_DPM_ADAPT_CHUNK elements.  A thread adds its elements in ascending order, the 256 threads fold in one
 *                          fixed tree: row n is bitwise the same in any batch and at any address.
 *   mmd_dpm_adapt_control  one workgroup, after both streams' close.  Per sample (batch != 0: for the whole batch, the reference's
 *                          rule) in fp64: sum the chunks of each stream in ascending order, E = max over streams of
 *                          (float)sqrt(sum / per); accept iff E <= 1: s = t, lambda_s = lambda(s); h = min(theta h E^(-1/2), lambda_0 -
 *                          lambda_s); done iff |s - t_0| <= t_err.  Then everything the next trial reads: t and s1 by piecewise-linear
 *                          interpolation in log_alpha (fp64 [T], log alpha at t_i = (i + 1) / T; sigma^2 = -expm1(2 log alpha)); the
 *                          model timesteps of s and s1, ((float)t - 1/T) * T truncated, each operation in fp32; the fp32 rows, each
 *                          rounded once from fp64; the row indices; the counters; status = {samples not done, fault}.  A non-finite
 *                          sum or E sets the fault bit (kept until the next init) and the flag REJECT and changes nothing else.
 *                          mode 1 (init): s = t_T, h = h_init, counters 0, flag IDLE, the first trial's rows; reads no partial sums.
 *                          state  fp64 [N][MMD_ADAPT_STATE_WORDS] (MMD_ADAPT_S_*)      cnt  int32 [N][4] (MMD_ADAPT_C_*)
 *                          itab   int64 [3][N] = k (n, or -1 when done), model timestep of s, of s1
 *                          ftab   fp32 [16][N]: rows 0-5 the open table (cx, ce at s; a0, a1, b0, b1), 6-11 the close table (cx, ce at
 *                                 s1; c0, c1, c2; 0), 12-13 alpha, sigma at s, 14-15 alpha, sigma at s1 (mmd_cond_replace's tables)
 *                          params fp64 [MMD_ADAPT_PARAMS] (MMD_ADAPT_P_*): the tolerances live in device memory, not in the launch
 *   mmd_dpm_adapt_commit   per sample by cnt's flag: ACCEPT PREV = LO; REJECT x = XB; IDLE nothing.
 *   mmd_dpm_adapt_time     dst[n] = src[n], int64 [N]: a row of model timesteps into the network's timestep buffer, which both
 *                          evaluations of a trial share (8 N bytes need not be the 16-byte rows mmd_copy2d moves). */
#define MMD_DPM_ADAPT_CHUNK 4096
#define MMD_ADAPT_PARAMS 8
#define MMD_ADAPT_P_ATOL 0
#define MMD_ADAPT_P_RTOL 1
#define MMD_ADAPT_P_THETA 2
#define MMD_ADAPT_P_TERR 3
#define MMD_ADAPT_P_HINIT 4
#define MMD_ADAPT_P_TT 5
#define MMD_ADAPT_P_T0 6
#define MMD_ADAPT_STATE_WORDS 8
#define MMD_ADAPT_S_S 0
#define MMD_ADAPT_S_H 1
#define MMD_ADAPT_S_LAM 2
#define MMD_ADAPT_S_T 3
#define MMD_ADAPT_S_S1 4
#define MMD_ADAPT_S_E 5
#define MMD_ADAPT_S_LAM0 6
#define MMD_ADAPT_S_SPARE 7
#define MMD_ADAPT_C_ATTEMPTS 0
#define MMD_ADAPT_C_ACCEPTED 1
#define MMD_ADAPT_C_FLAG 2
#define MMD_ADAPT_C_DONE 3
#define MMD_ADAPT_FLAG_REJECT 0
#define MMD_ADAPT_FLAG_ACCEPT 1
#define MMD_ADAPT_FLAG_IDLE 2
int64_t mmd_dpm_adapt_chunks(int64_t per_sample);
int mmd_dpm_adapt_open(float* x, const float* src, int form, float* XB, float* MS, float* LO, const float* s, float max_val,
                       const float* tab, const int64_t* k, int rows, int N, int F, int C, int Cm, int HW, void* stream);
int mmd_dpm_adapt_close(float* x, const float* src, int form, const float* XB, const float* MS, const float* LO, const float* PREV,
                        const float* s, float max_val, const float* tab, const int64_t* k, int rows, const double* params, double* partial,
                        int N, int F, int C, int Cm, int HW, void* stream);
int mmd_dpm_adapt_control(int mode, int batch, const double* params, const double* log_alpha, int T, const double* partial_v, int chunks_v,
                          int64_t per_v, const double* partial_a, int chunks_a, int64_t per_a, double* state, int64_t* itab, int32_t* cnt,
                          float* ftab, int32_t* status, int N, void* stream);
int mmd_dpm_adapt_commit(float* x, const float* XB, float* PREV, const float* LO, const int32_t* cnt, int N, int64_t per_sample,
                         void* stream);
int mmd_dpm_adapt_time(const int64_t* src, int64_t* dst, int N, void* stream);
/* SR model input (image_unet.py:704-715): out [N,2C,H,W] = concat(x [N,C,H,W], bilinear(low [N,C,h,w] -> H x W)), fp32. */
int mmd_bilinear_concat(const float* x, const float* low, float* out, int N, int C, int H, int W, int h, int w, void* stream);
/* The same tensor as channels-last rows [(n, y, x), Cpad] in `dtype` (channels 2C..Cpad zero): feeds the SR stem as an implicit GEMM. */
int mmd_bilinear_concat_rows(int dtype, const float* x, const float* low, void* out, int N, int C, int H, int W, int h, int w, int Cpad,
                             void* stream);
/* Gradient of sum_n(dmse[n] mse[n] + dvb[n] vb[n]) of mmd_loss_terms w.r.t. the model output (same layout, fp32): the mean channels
 * get the mse gradient only (the vb term detaches the mean, gd:1147-1151), the variance channels the KL / decoder-NLL gradient. */
int mmd_loss_terms_bwd(const float* x0, const float* xt, const float* model_out, const float* target, const float* tables,
                       const int64_t* t, int T, int N, int F, int C, int HW, int flags, float vb_scale, const float* dmse,
                       const float* dvb, float* g_model_out, void* stream);
/* backward of mmd_attn_small_fwd (temporal attention): dQKV rows [dq | dk | dv], same slice geometry. */
int mmd_attn_small_bwd(int dtype, const void* QKV, int64_t ld, const void* dO, int64_t lddo, void* dQKV, int64_t ldd, int C, int heads,
                       int S, int Tn, int inner, int64_t outer_stride, int64_t inner_stride, int64_t tstride, void* stream);
/* out = silu(x) (dy NULL) or dy*silu'(x); d(mse loss)/d(out); AdamW (+EMA, nn.py:128-138) on flat fp32 buffers. */
int mmd_timestep_embedding(const void* t, int t_kind, int N, int dim, float* out, void* stream);   /* nn.py:192-210 */
int mmd_silu(int dtype, const void* x, const void* dy, void* out, int64_t n, void* stream);
int mmd_dropout(int dtype, const void* x, const uint8_t* mask, float scale, void* out, int64_t n, void* stream);   /* nn.Dropout, unet:376 */
int mmd_mse_grad(const float* out, const float* target, const float* w, float* g, int N, int64_t per_sample, void* stream);
int mmd_adamw_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, float ema_rate, void* stream);

/* --- training step guard: gradient / parameter norms, non-finite skip and clipping decided ON THE DEVICE (reference
 * fp16_util.py:188-236: norms logged per step, took_step = False on a non-finite gradient norm, EMA only if took_step).
 * Three ordinary launches in stream order; none communicates between its blocks and every sum has a fixed order (double), so
 * the results are bitwise repeatable.  The host reads the control block only when it logs. */
#define MMD_STEP_CHUNK 16384     /* longest chunk of the chunk table, in elements */
#define MMD_STEP_MAX_EMA 4
struct mmd_step_ctrl {           /* 64 bytes, device memory, zero-initialised by the caller */
  double cum_grad_norm;          /* never-reset sums over the TAKEN steps: interval means come from differencing two reads */
  double cum_param_norm;
  int64_t cum_count;
  float grad_norm;               /* this step, before clipping; rounded once from the double sqrt */
  float param_norm;              /* the parameters the step is applied to (before the update) */
  float clip_coef;               /* 1, or max_grad_norm / (grad_norm + 1e-6) when the norm exceeds max_grad_norm > 0 */
  float bc1, bc2;                /* 1 - beta^steps_taken of the step about to be applied */
  int32_t took_step;             /* 1 iff the gradient sum of squares is finite */
  int32_t steps_taken;           /* incremented only when took_step */
  int32_t skipped_total;
  int32_t first_bad_param;       /* this step: lowest parameter whose gradient sum is non-finite, else -1 */
  int32_t last_bad_param;        /* first_bad_param of the most recent skipped step (the caller initialises both to -1) */
};
int mmd_step_ctrl_bytes(void);   /* sizeof(struct mmd_step_ctrl) as the library was compiled (host only) */
/* partial[c] = { sum g^2, sum p^2 } (double) over chunk c = elements [chunk_lo[c], chunk_lo[c] + chunk_len[c]) of the flat fp32
 * buffers g / p (p nullable: 0), one block per chunk; chunk starts need only 4-byte alignment.  A chunk that leaves [0, n) is
 * clipped to it.  An fp32 square cannot overflow a double, so a sum is non-finite exactly when one of its elements is. */
int mmd_sumsq_chunks(const float* g, const float* p, int64_t n, const int64_t* chunk_lo, const int32_t* chunk_len, int nchunks,
                     double* partial, void* stream);
/* One block: param_sumsq[i] = fold of the chunks param_first_chunk[i] .. param_first_chunk[i + 1] - 1 in ascending order, the
 * totals a fixed-order fold of those; then the control block is advanced by one step (see the struct). */
int mmd_step_control(const double* partial, const int32_t* param_first_chunk, int P, double* param_sumsq, float max_grad_norm,
                     float beta1, float beta2, struct mmd_step_ctrl* ctrl, void* stream);
/* AdamW + up to MMD_STEP_MAX_EMA EMA copies (NULL = absent) in one launch on g * ctrl->clip_coef with the bias corrections of
 * ctrl; every thread returns at once when ctrl->took_step is 0 (p, m, v and the EMA copies stay bitwise what they were). */
int mmd_adamw_step_guarded(float* p, const float* g, float* m, float* v, float* ema0, float* ema1, float* ema2, float* ema3,
                           float rate0, float rate1, float rate2, float rate3, int64_t n, float lr, float beta1, float beta2,
                           float eps, float weight_decay, const struct mmd_step_ctrl* ctrl, void* stream);

#ifdef __cplusplus
}
#endif
#endif
