/*
 * showtell_hip.h -- C ABI of libshowtell_hip.so, the MI355X (gfx950) kernels of the
 * show-tell captioning hot path.
 *
 * The reference (guptakhil/show-tell) has no FFI layer: its hot path is the Python
 * nn.Module surface (cnn.py, rnn.py, Attention/rnn_attn.py, LSTM/rnn_lstm.py) whose
 * arithmetic is delegated to torch / cuDNN / cuBLAS.  Each entry point below
 * replaces one such delegated call site (cited as file:line of /root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream);
 *   - every function returns 0 on success, non-zero on error;
 *     st_last_error() returns a thread-local message;
 *   - nothing is allocated, freed or synchronised inside a call (graph-capturable);
 *     workspaces are caller-provided;
 *   - dtype codes: ST_F32 = 0, ST_BF16 = 1.  bf16 tensors are raw uint16 bit patterns.
 *   - activations are NHWC ("pixel-major"), weights are [Cout][KH][KW][Cin].
 */
#ifndef SHOWTELL_HIP_H
#define SHOWTELL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_F32 0
#define ST_BF16 1

#define ST_CELL_GRU 0
#define ST_CELL_LSTM 1

const char* st_last_error(void);
int st_version(void);

/* ------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / dense projection on MFMA.
 *   y[m][n] = sum_k x_gather[m][k] * w[n][k]        m = (b,ho,wo), k = (kh,kw,c)
 * Sliding-window form: KW == 1, pad == 0 and ldx < Cin with Cin % ldx == 0 reads Cin consecutive elements
 * starting at pixel (hi, wi), i.e. Cin/ldx neighbouring pixels of one row as one tap (the space-to-depth
 * stem); the caller's rows must be wide enough: (Wo-1)*stride + Cin/ldx <= Win.
 * Replaces: torchvision conv2d inside cnn.py:46 / cnn_attn.py:46 (cuDNN conv),
 * nn.Linear at cnn.py:49, rnn.py:33 and the GRU input projections inside rnn.py:32.
 * A plain GEMM is the case KH=KW=1, Hin=Win=Ho=Wo=1, B=M, Cin=K.
 * Epilogue (all optional, in this order):  v = acc + bias[n];  stats[n] += v, stats[N+n] += v*v
 * (fp32 atomics, batch-norm statistics; with stats_replicas = R > 1 the buffer is [R][2N] and pixel tile t
 * adds into replica t % R -- same-address float atomics serialise at the memory side, ~25 ns each, so layers
 * with thousands of pixel tiles spread them; the consumer sums the replicas);  v = v*scale[n] + shift[n];  v += residual[m][n];
 * v = max(v,0) if relu;  y = (accumulate ? y : 0) + v.
 * Requirements: Cin, ldx, ldw multiples of 8 (bf16) / 4 (f32); ldy multiple of 4.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const void* x;        /* [B,Hin,Win,ldx] dtype                                    */
  const void* w;        /* [N][ldw] dtype, K = KH*KW*Cin contiguous                 */
  void* y;              /* [M][ldy] out_dtype, M = B*Ho*Wo                          */
  const float* bias;    /* [N] or NULL                                              */
  const float* scale;   /* [N] or NULL                                              */
  const float* shift;   /* [N] or NULL                                              */
  const void* residual; /* [M][ldy] out_dtype or NULL                               */
  float* stats;         /* [2N] or NULL                                             */
  int dtype, out_dtype;
  int B, Hin, Win, Cin, Ho, Wo, N, KH, KW, stride, pad;
  int ldx, ldw, ldy;
  int relu, accumulate;
  int Cin_logical;      /* 0 = Cin; the un-padded channel count (profiler FLOP accounting) */
  int k_order;          /* 0: w is [N][KH][KW][Cin]; 1: w is [N][Cin/CH][KH][KW][CH], CH = 128 bytes of channels */
  int stats_replicas;   /* 0/1: stats is [2N]; R > 1: stats is [R][2N] (see above)               */
  /* Optional input transform (train-mode bottleneck, cnn.py:46): x is the RAW output of the producing conv and the
   * A operand becomes relu(batchnorm(x)) with batch statistics in_stats = [sum | sumsq] over in_count rows -- the
   * producer's normalise pass is absorbed by this conv.  Needs Cin % 64 == 0 (bf16) / 32 (f32).  NULL = off. */
  const float* in_stats; const float* in_gamma; const float* in_beta; float in_count, in_eps;
  int split_k;          /* > 1 (plain GEMM, fp32 output, K % (split_k*64|32) == 0): K is cut into split_k slices that run as
                         * one grouped launch and add their tiles with fp32 atomics -- for products with few output tiles */
} st_conv_desc;

int st_conv(const st_conv_desc* d, void* stream);
/* n <= 12 independent problems of identical shape, dtype and options (only the pointers differ) as ONE launch: the
 * per-layer weight-gradient GEMMs of the decoder backward (autograd of nn.GRU, main.py:151) are 48 tiles each. */
int st_conv_batch(const st_conv_desc* d, int n, void* stream);
/* Which kernel the calling thread's last st_conv / st_conv_batch launch was: a thread-local record written just before the
 * launch, for tests that assert the route a shape is meant to take.  It changes no launch.  out[8] =
 *   [0] main loop: 0 register-staged two-buffer, 1 single-buffer DMA, 2 three-buffer DMA
 *   [1] BM  [2] BN: tile rows (pixels) and columns (channels)   [3] waves per workgroup   [4] KC: 16-byte chunks per tile row, 8 | 4
 *   [5] MODE: 0 generic tap walk, 1 whole K tiles inside one tap, 2 the same with the input transform
 *   [6] group members of the launch (st_conv_batch's n, split_k's slices, else 1)   [7] 1: fp32 atomics into y (split-K), else 0
 * all -1 before the thread's first launch.  Returns the number of such launches the thread has made; a refused call (non-zero
 * return of st_conv / st_conv_batch) launches nothing, so it leaves both the record and the count as they were.  out may be NULL. */
int st_conv_last_route(int* out);

/* ------------------------------------------------------------------------------------
 * Token-contraction GEMM (csrc/gemm_tn.hip), bf16 operands, fp32 result:
 *   c[m][n] (+)= sum_k a[k][m] * b[k][n]            a: [K][lda], b: [K][ldb], both ROW-major, K the slow axis
 * The parameter gradients of the decoder backward (autograd of nn.Linear / nn.GRU / nn.LSTM, main.py:151) contract over
 * the tokens, which is the slow axis of every operand as stored; both tiles are read as they lie and transposed on the way
 * out of LDS (ds_read_b64_tr_b16), so no K-major copy is made.  One workgroup owns an output tile over the whole of K:
 * no atomics, two identical calls give bit-identical results.
 * Requirements: dtype ST_BF16; lda >= M, ldb >= N, both multiples of 8; a and b 16-byte aligned; ldc >= N.
 * Columns M .. lda of a and N .. ldb of b may hold anything.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const void* a;        /* [K][lda] bf16                                                                   */
  const void* b;        /* [K][ldb] bf16, or the matrix b_row indexes                                      */
  float* c;             /* [M][ldc] fp32                                                                   */
  const int* b_row;     /* [K] or NULL: row k of b is b[b_row[k]], a row of zeros where b_row[k] < 0       */
  const int* b_live;    /* [K] or NULL (needs b_row): row k of b is zero where b_live[k] <= 0, b_row[k] is
                         * then not read as an index (st_packed_seq.rows_t / prev_row: h_{t-1} of a token)   */
  float* colsum0;       /* [M] or NULL: colsum0[m] += sum_k a[k][m] (always added, whatever `accumulate`)   */
  float* colsum1;       /* [M] or NULL: the same sums added to a second vector                             */
  int dtype;
  int M, N, K;
  int lda, ldb, ldc;
  int accumulate;       /* 0: c = product; 1: c += product                                                 */
} st_gemm_tn_desc;
/* n <= 12 problems of any mix of shapes as ONE launch */
int st_gemm_tn_batch(const st_gemm_tn_desc* d, int n, void* stream);

/* ------------------------------------------------------------------------------------
 * Image-resident 3x3 stride-1 pad-1 convolution, bf16 (the conv2 of torchvision's Bottleneck / the convs of BasicBlock
 * behind `self.model(x)`, reference cnn.py:46 / cnn_attn.py:46; csrc/conv_img.hip).  A workgroup keeps a band of one
 * image (+ zero halo) in LDS for all nine taps, the filter bank streams fragment-major from HBM/L2 straight into MFMA
 * operand registers, no barrier in the K loop.  x: [B][H][W][C] bf16 (dense), y: [B][H][W][N] bf16 (dense),
 * w_frag: st_pack_conv_weight_frag(.., ntw = st_conv3x3_img_supported(H, W, C, N)).
 *   in_stats != NULL: x is the RAW output of the producer convolution; the fill applies relu(batchnorm(x)) with the
 *                     producer's batch statistics ([sum | sumsq] over in_count rows) once per element (bn1 + ReLU of
 *                     the Bottleneck in train mode, main.py:125) -- the separate normalise pass disappears.
 *   stats != NULL   : per-channel [sum(N) | sumsq(N)] of the fp32 results are added (stats_replicas as in st_conv_desc;
 *                     the replica is (image, band) %% R).
 *   scale/shift/relu: eval-mode epilogue y = relu?(acc * scale + shift).
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const void* x; const void* w_frag; void* y;
  float* stats; int stats_replicas;
  const float* scale; const float* shift; int relu;
  const float* in_stats; const float* in_gamma; const float* in_beta; float in_count; float in_eps;
  int B, H, W, C, N;
  int in_stats_replicas;   /* 0/1: in_stats is [2C]; R > 1: [R][2C], summed by the kernel (no reduction launch in between) */
} st_conv3x3_img_desc;
/* > 0: supported, the value is the LAYOUT CODE the weights must be packed with (st_pack_conv_weight_frag's `ntw` argument:
 * low byte = 16-channel tiles per wave, bits 8.. = channel halves of the K order); 0: use st_conv */
int st_conv3x3_img_supported(int H, int W, int C, int N);
int st_conv3x3_img(const st_conv3x3_img_desc* d, void* stream);
/* The stride-2 siblings (3x3, pad 1, stride 2: conv2 of the first block of layer2 / layer3 / layer4; csrc/conv_s2.hip): a K-streaming implicit
 * GEMM with gathered rows, (C, N) in {(128, 128), (256, 256), (512, 512)}.  Same descriptor (H, W = input size, y: [B][(H-1)/2+1][(W-1)/2+1][N]);
 * w_frag: st_pack_conv_weight_frag(.., KH = KW = 3, ntw = st_conv3x3_s2_supported(C, N)). */
int st_conv3x3_s2_supported(int C, int N);
int st_conv3x3_s2(const st_conv3x3_img_desc* d, void* stream);
/* ------------------------------------------------------------------------------------
 * Pointwise (1x1, stride 1 or 2) convolution with the filter slice held in registers, bf16, C <= 512 input channels
 * (conv3 / downsample of torchvision's Bottleneck and the narrow conv1s, reference cnn.py:46; csrc/conv_img.hip).
 * x: [B][Hin][Win][C] bf16 (dense), y: [B][Ho][Wo][N] bf16 with Ho = (Hin - 1) / stride + 1;
 * w_frag: st_pack_conv_weight_frag(.., KH = KW = 1, ntw = st_conv1x1_wreg_supported(C, N)).
 * in_stats / stats / scale / shift / relu as in st_conv3x3_img_desc.  residual ([B][Ho][Wo][N] bf16, the Bottleneck's identity): the
 * eval-mode conv3 epilogue y = relu(conv(x) * scale + shift + residual) -- needs scale / shift, stride 1, no statistics (st_conv1x1_wreg
 * and the stride-1 forms of st_conv1x1_astat; st_conv1x1_kstream has none).  y may be NULL in train mode (stats given): only the
 * statistics of the output are produced.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const void* x; const void* w_frag; void* y; const void* residual;
  float* stats; int stats_replicas;
  const float* scale; const float* shift; int relu;
  const float* in_stats; const float* in_gamma; const float* in_beta; float in_count; float in_eps; int in_stats_replicas;
  int B, Hin, Win, C, N, stride;
} st_conv1x1_wreg_desc;
int st_conv1x1_wreg_supported(int C, int N);
int st_conv1x1_wreg(const st_conv1x1_wreg_desc* d, void* stream);
/* The long-K sibling (C = 1024 / 2048 input channels, N a multiple of 256: the conv1 of the layer3 / layer4 Bottlenecks): a
 * workgroup owns 112 rows x 256 channels and streams K through a padded LDS ring (activations) and a register ring
 * (fragment-major filters, ntw = 4).  Same descriptor; in_stats and residual must be NULL. */
int st_conv1x1_kstream_supported(int C, int N);
int st_conv1x1_kstream(const st_conv1x1_wreg_desc* d, void* stream);
/* conv1 of a Bottleneck fused with the PREVIOUS block's end (torchvision Bottleneck.forward: out = relu(bn3(conv3(..)) + identity),
 * then the next block's conv1(out); reference cnn.py:46), train mode:
 *   x_out = relu(batchnorm(raw; f_stats, f_gamma, f_beta) + idn)   -- written once, it is the next identity
 *           idn = identity, or batchnorm(identity; id_stats, id_gamma, id_beta) when id_stats is given (the previous block had a
 *           downsample conv whose raw output is the identity; same count / eps as f_*)
 *   y     = x_out (*) w_frag (1x1 fragment-major weights, layout code st_conv1x1_kfuse_supported(C, N)),  stats += [sum | sumsq] of y
 * raw / identity / x_out: [rows][C] bf16 (x_out must not alias raw or identity), y: [rows][N] bf16.  Replaces one st_bn_act pass +
 * the conv1 launch.  C = 256 / 512 (layer1 / layer2 and the first conv1 of layer2 / layer3): the register-resident-filter kernel's
 * loader, same weights as st_conv1x1_wreg; C = 1024 -> N = 256: the K-streaming form (id_stats must be NULL; measured slower than the
 * separate pass, compiled only under ST_EXPERIMENTAL). */
typedef struct {
  const void* raw; const void* identity; void* x_out; const void* w_frag; void* y;
  float* stats; int stats_replicas;
  const float* f_stats; const float* f_gamma; const float* f_beta; float f_count; float f_eps; int f_stats_replicas;
  long rows; int C, N;
  const float* id_stats; const float* id_gamma; const float* id_beta; int id_stats_replicas;
} st_conv1x1_kfuse_desc;
int st_conv1x1_kfuse_supported(int C, int N);
int st_conv1x1_kfuse(const st_conv1x1_kfuse_desc* d, void* stream);
/* The 1024 -> 256 form as a producer / consumer workgroup (csrc/conv_kfuse8.hip): four waves multiply, four load / normalise / store; same
 * descriptor (id_stats must be NULL), same results bit for bit.  Measured a wash against st_bn_act + st_conv1x1_kstream (106.7 vs 108.0 us per
 * layer3 block); st_resnet_forward does not use it. */
#ifdef ST_EXPERIMENTAL   /* `make EXPERIMENTAL=1`: not part of the product library */
int st_conv1x1_kfuse8(const st_conv1x1_kfuse_desc* d, void* stream);
#endif
/* Block boundary of the 56 x 56 Bottlenecks in one pass over the wide tensors (csrc/conv_b2b.hip; train mode, bf16):
 *   x_out = relu(bn3(conv3(relu(bn2(raw2)))) + idn),   y = conv1_next(x_out)   (+ statistics of y)
 * conv3 (C1 = 64 -> C2 = 256) is RE-computed here from the narrow tensor raw2 [rows][64] instead of being written and read back;
 * its batch statistics (bn3_stats) come from a st_conv1x1_wreg call with y == NULL over the same raw2 / w3_frag.  idn = identity, or
 * batchnorm(identity; id_*) after a downsample conv.  w3_frag / w1_frag: the fragment-major copies st_conv1x1_wreg uses for the two
 * layers (C1 -> C2 and C2 -> N, N = 64 | 128).  Bit-identical to st_conv1x1_wreg -> st_bn_act -> st_conv1x1_wreg.  `count` rows went
 * into every statistic; x_out must not alias an input. */
typedef struct {
  const void* raw2; const void* w3_frag; const void* identity; void* x_out; const void* w1_frag; void* y;
  float* stats; int stats_replicas;
  const float* bn2_stats; const float* bn2_gamma; const float* bn2_beta; int bn2_replicas;
  const float* bn3_stats; const float* bn3_gamma; const float* bn3_beta; int bn3_replicas;
  const float* id_stats; const float* id_gamma; const float* id_beta; int id_replicas;
  float count; float eps;
  long rows; int C1, C2, N;
} st_conv_b2b_desc;
/* Layout contract (the kernel indexes the fragments with fixed tile permutations): w3_frag packed with ntw = 2, w1_frag with
 * ntw = N / 64 -- what st_conv1x1_wreg_supported returns for these layers today; a caller that packs another ntw gets wrong channels. */
int st_conv_b2b_supported(int C1, int C2, int N);
int st_conv_b2b(const st_conv_b2b_desc* d, void* stream);
/* conv3 of a 14 x 14 Bottleneck (C1 = 256 -> C2 = 1024) or a 28 x 28 one (128 -> 512), the block's end, and conv1 of the NEXT block
 * (C2 -> N = C1) in one kernel (csrc/conv_c3c1.hip; torchvision Bottleneck.forward twice over, reference cnn.py:46):
 *   x_out = relu(bn3(conv3(a2)) + identity),   y = conv1_next(x_out)
 * conv3's output channels are conv1's K dimension: each finished 128-channel chunk of x is stored once AND is one K-slab of conv1
 * (through LDS); x is never read back.  Replaces st_conv1x1_astat + st_bn_act + st_conv1x1_kstream (28 x 28: st_conv1x1_wreg +
 * st_bn_act + st_conv1x1_wreg).
 *   train (bn3_stats given): a2 = relu(batchnorm(x2; bn2_*)) (bn2_stats NULL: x2 is already normalised); bn3 from the batch statistics of
 *     conv3's output, which a STATISTICS-ONLY st_conv1x1_astat (28 x 28: st_conv1x1_wreg) call (y == NULL) over the same x2 / w3_frag
 *     produces first; `stats` receives
 *     [sum | sumsq] of y.  x_out and y are bit-identical to the three-kernel path.
 *   eval (scale3 / shift3 / scale1 / shift1 given, no statistics): a2 = x2, x_out = relu(conv3 * scale3 + shift3 + identity),
 *     y = conv1(x_out) * scale1 + shift1 (ReLU if relu1).
 * x2: [rows][C1], identity / x_out: [rows][C2], y: [rows][N], all bf16.  w3_frag: st_pack_conv_weight_frag(ntw = 2) (the layout
 * st_conv1x1_astat / st_conv1x1_wreg use for conv3), w1_frag: ntw = N / 64 (st_conv1x1_kstream's | st_conv1x1_wreg's for that conv1). */
typedef struct {
  const void* x2; const void* w3_frag; const void* identity; void* x_out; const void* w1_frag; void* y;
  float* stats; int stats_replicas;
  const float* bn2_stats; const float* bn2_gamma; const float* bn2_beta; int bn2_replicas;
  const float* bn3_stats; const float* bn3_gamma; const float* bn3_beta; int bn3_replicas;
  float count; float eps;
  const float* scale3; const float* shift3; const float* scale1; const float* shift1; int relu1;
  long rows; int C1, C2, N;
  /* train, optional: the identity is the RAW output of a downsample conv with these batch statistics (the block behind it):
   * x_out = relu(bn3(conv3) + batchnorm(identity; id_*)), st_bn_act's res_bn form */
  const float* id_stats; const float* id_gamma; const float* id_beta; int id_replicas;
} st_conv_c3c1_desc;
int st_conv_c3c1_supported(int C1, int C2, int N);
int st_conv_c3c1(const st_conv_c3c1_desc* d, void* stream);
/* The activation-stationary sibling for (C, N) = (256, 1024) / (512, 2048) (conv3 of the layer3 / layer4 Bottlenecks): a
 * workgroup keeps its 112 x C rows in LDS (producer's BatchNorm + ReLU applied once per element) and walks all N output
 * channels barrier-free, the epilogue of one 128-channel chunk under the next chunk's MFMAs.  Same descriptor (weights packed with the
 * layout code st_conv1x1_astat_supported returns), stride 1, residual NULL. */
int st_conv1x1_astat_supported(int C, int N);
int st_conv1x1_astat(const st_conv1x1_wreg_desc* d, void* stream);

/* [Cout][Cin][KH][KW] fp32 (torch layout) -> fragment-major bf16: element ((T * KS + ks) * 64 + lane) * 8 + j is
 * w[ch(T, lane & 15)][k = 32 ks + 8 (lane >> 4) + j] with k = (kh * KW + kw) * Cin + c and
 * ch(T, r) = (T / ntw) * 16 ntw + 4 ntw (r / 4) + 4 (T %% ntw) + r %% 4: one coalesced 1-KiB load is one MFMA operand
 * (16 output channels x 32 K), and a wave that owns ntw tiles ends with 4 ntw consecutive channels per lane. */
int st_pack_conv_weight_frag(const float* w, void* out, int Cout, int Cin, int KH, int KW, int ntw, void* stream);

/* Launch profiler for bench.py's roofline: HIP events around every convolution launch on its stream.
 * st_prof_collect fills 32-entry arrays indexed by kernel variant (0: bf16 128x128 tile family,
 * 1: bf16 128x64, 2: bf16 64x128, 3: 256x128, 4..7 the same for f32, 8..19: the csrc/conv_img.hip kernels, one slot per kernel symbol
 * (csrc/prof.h)); synchronise the device first. */
int st_tune(int reserved, int kc, int w8);   /* main-loop variant knobs for tools/bench_conv.py (row chunk count 4|8, block shape); -1 = keep */
int st_prof_enable(int on);
/* debug aid: per-block phase timestamps of st_conv launches (tools/conv_stamps.py); NULL = off (default) */
int st_debug_stamps(unsigned long long* buf);
int st_prof_collect(double* ms, double* flops, long* launches);

/* ------------------------------------------------------------------------------------
 * Batch-norm apply (+ residual)(+ ReLU), NHWC, fused elementwise pass.
 * Replaces: nn.BatchNorm2d + ReLU + residual add inside torchvision's Bottleneck
 * (cnn.py:46).  Train mode (main.py:125): stats = [sum | sumsq] from st_conv, count = B*H*W.
 *   scale = gamma*rsqrt(var+eps), shift = beta - mean*scale   (biased var)
 *   y = relu?( x*scale+shift + (res ? (res_stats ? res*rscale+rshift : res) : 0) )
 * Eval mode: pass stats = NULL and running_mean/var.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  const void* x; void* y; const void* res;      /* [rows][C] dtype                  */
  const float* stats;  const float* gamma; const float* beta;
  const float* running_mean; const float* running_var;      /* eval mode            */
  const float* res_stats; const float* res_gamma; const float* res_beta;
  const float* res_running_mean; const float* res_running_var;
  int res_bn;          /* 1: residual goes through its own BN (downsample branch)   */
  int dtype; long rows; int C; float count; float eps; int relu;
  int stats_replicas, res_stats_replicas;   /* 0/1: [2C]; R > 1: [R][2C], summed here (st_conv_desc.stats_replicas) */
} st_bn_act_desc;

int st_bn_act(const st_bn_act_desc* d, void* stream);

/* running_mean/var momentum update from [sum|sumsq] (unbiased var), nn.BatchNorm semantics */
int st_bn_update_running(const float* stats, float* running_mean, float* running_var,
                         int C, float count, float momentum, void* stream);

/* NCHW fp32 images (utils.py:61-77 layout) -> NHWC dtype with channels zero-padded to Cpad */
int st_nchw_to_nhwc(const float* x, void* y, int dtype, int B, int C, int H, int W, int Cpad, void* stream);
/* NCHW fp32 RGB images (even H, W) -> 2x2 space-to-depth NHWC [B][H/2+3][W/2+3][16] dtype: blocked pixel (p,q) holds
 * rows 2(p-2)+dy, cols 2(q-2)+dx as channel (dy*2+dx)*3+c; channels 12..15 and the border (2 before, 1 after) are zero.
 * With st_stem_weight_s2d the torchvision stem (7x7 s2 p3, cnn.py:46) becomes st_conv's sliding-window form:
 * Hin=H/2+3, Win=W/2+3, Cin=64, ldx=16, KH=4, KW=1, stride=1, pad=0, Ho=H/2, Wo=W/2, ldw=256. */
int st_nchw_to_s2d16(const float* x, void* y, int dtype, int B, int H, int W, void* stream);
/* packed stem weights [64][7][7][Cpad] dtype (st_pack_conv_weight, k_order 0) -> [64][4][4][16] dtype for the blocked image */
int st_stem_weight_s2d(const void* w, void* out, int dtype, int Cpad, void* stream);
/* NHWC dtype -> (B,C,H*W) fp32, the layout cnn_attn.py:49 returns */
int st_nhwc_to_ncp_f32(const void* x, float* y, int dtype, int B, int HW, int C, void* stream);
/* 3x3 stride-2 pad-1 max pool NHWC (torchvision resnet maxpool, cnn.py:46) */
int st_maxpool3x3s2(const void* x, void* y, int dtype, int B, int H, int W, int C, void* stream);
/* y = maxpool3x3s2(relu(batchnorm(x))): the stem's bn1 + relu + maxpool of torchvision's resnet in one pass
 * (train: stats = [sum|sumsq] over `count` rows; eval: stats NULL, running buffers).  C must divide 2048 (bf16) / 1024 (f32). */
int st_maxpool3x3s2_bn(const void* x, void* y, int dtype, int B, int H, int W, int C,
                       const float* stats, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, float count, float eps, void* stream);
/* The bf16 stem in one kernel (csrc/conv_stem.hip): conv1 7x7/2 (+ BatchNorm statistics) + maxpool 3x3/2 of torchvision's resnet
 * (the first four modules of the reference's `self.model`, cnn.py:46); replaces st_conv on the blocked image + st_maxpool3x3s2(_bn).
 *   x_s2d : st_nchw_to_s2d16's blocked image [B][H/2+3][W/2+3][16] bf16;  w_frag : st_stem_weight_frag(st_stem_weight_s2d(..)) (64 x 256)
 *   y     : [B][PH][PW][64] bf16, PH = (H/2 - 1)/2 + 1
 * train (scale == NULL): y = pool(raw conv output) with MAX on channels with gamma >= 0 and MIN on the others -- the consumer applies
 *   relu(bn1(.)) to y (monotone per channel, so this IS maxpool(relu(bn1(conv)))); stats[replica][sum(64) | sumsq(64)] += the raw
 *   convolution output's sums over all B x H/2 x W/2 positions (fp32 accumulators), replica = workgroup %% stats_replicas.
 * eval (scale, shift = folded bn1): y = maxpool(relu(conv * scale + shift)). */
typedef struct {
  const void* x_s2d; const void* w_frag; void* y;
  float* stats; int stats_replicas;
  const float* gamma;
  const float* scale; const float* shift;
  int B, H, W;
} st_stem_conv_pool_desc;
int st_stem_conv_pool(const st_stem_conv_pool_desc* d, void* stream);
int st_stem_weight_frag(const void* w_s2d, void* out, void* stream);
/* == st_stem_weight_frag(st_stem_weight_s2d(w_packed, bf16, Cpad)) in one launch (what st_resnet_forward runs per forward) */
int st_stem_weight_frag_packed(const void* w_packed, int Cpad, void* out, void* stream);
/* global average pool NHWC -> [B][C] (adaptive avgpool, cnn.py:34) */
int st_global_avgpool(const void* x, void* y, int dtype, int out_dtype, int B, int HW, int C, void* stream);

/* Device-side input transform of a minibatch (utils.py:84-88: Resize((224,224)) -> RandomHorizontalFlip ->
 * RandomVerticalFlip -> ToTensor -> Normalize, applied per image at utils.py:45-47 and stacked at utils.py:68).
 * Resize is Pillow's 8-bit BILINEAR resample, bit for bit (horizontal pass, uint8 intermediate, vertical pass);
 * the coin flips are the caller's; `lut` = the caller's float32 table ((v / 255) - mean[c]) / std[c].
 * Limits: out_h, out_w <= 320; down-scaling factors up to 19 per axis. */
typedef struct st_image_batch_desc {
  const uint8_t* src;      /* device: the batch's RGB images, HWC uint8, back to back */
  int64_t src_bytes;       /* size of src (offset[b] + 3 * height[b] * width[b] <= src_bytes for every b) */
  const int64_t* offset;   /* device [batch]: byte offset of image b in src */
  const int32_t* height;   /* device [batch] */
  const int32_t* width;    /* device [batch] */
  const int32_t* flip;     /* device [batch]: bit 0 = left-right, bit 1 = top-bottom; NULL = no flips */
  int batch;
  int max_height, max_width; /* bounds of height[] / width[] (sizes the launch and the scratch) */
  int out_h, out_w;
  const float* lut;        /* device [3][256] */
  uint8_t* tmp;            /* device scratch, batch * max_height * out_w * 3 bytes */
  float* out;              /* device (batch, 3, out_h, out_w) fp32: the `images` tensor of utils.py:68 */
  uint8_t* out_u8;         /* optional device (batch, out_h, out_w, 3): the resized + flipped pixels before ToTensor */
} st_image_batch_desc;
int st_image_transform(const st_image_batch_desc* d, void* stream);

/* Generic helpers */
int st_cast(const void* x, void* y, int from_dtype, int to_dtype, long n, void* stream);
/* y[c][r] = x[r][c]; y has leading dimension ldy >= rows, pad columns zero-filled */
int st_transpose(const void* x, void* y, int dtype, int rows, int cols, int ldx, int ldy, void* stream);
/* the same, and colsum[c] += sum_r x[r][c] (fp32 atomics) from the tile already in LDS: the bias gradient that goes with
 * every K-major copy of a gradient matrix in the decoder backward (autograd of nn.Linear / nn.GRU, main.py:151) */
int st_transpose_colsum(const void* x, void* y, float* colsum, int dtype, int rows, int cols, int ldx, int ldy, void* stream);
/* n <= 12 matrices of identical shape in one launch (the same operand of every decoder layer); colsum may be NULL or hold
 * NULL entries.  With rows_t / prev_row (packed-sequence tables, st_packed_seq) output row r is read from source row
 * prev_row[r], zero where rows_t[r] == 0: h_{t-1} of every token transposed straight out of the layer output. */
int st_transpose_batch(const void* const* x, void* const* y, float* const* colsum, int n, int dtype, int rows, int cols,
                       int ldx, int ldy, const int* rows_t, const int* prev_row, void* stream);
/* conv weight repack: [Cout][Cin][KH][KW] fp32 (torch layout) -> [Cout][KH][KW][Cpad] dtype (k_order 0)
 * or [Cout][Cpad/CH][KH][KW][CH] with CH = 64 (bf16) / 32 (f32) channels (k_order 1, see st_conv_desc) */
int st_pack_conv_weight(const float* w, void* out, int dtype, int Cout, int Cin, int KH, int KW, int Cpad, int k_order, void* stream);

/* ------------------------------------------------------------------------------------
 * ResNet-{18,34,50,101,152} backbone forward, one call (torchvision children()[:-1] /
 * [:-2]; reference cnn.py:23-34,46 and cnn_attn.py:23-34,46-49).
 * Layers are indexed in forward order: stem conv, then per block conv1, conv2, [conv3],
 * [downsample]; st_resnet_conv_info gives geometry and the element offsets of layer i in
 * the packed weight buffer ([Cout][KH][KW][Cin_padded], dtype) and in the concatenated
 * BatchNorm arrays (gamma, beta, running_mean, running_var: fp32, one entry per channel).
 * st_resnet_create returns 2 with the reference's ValueError text (cnn.py:33) for an
 * unknown version.  Outputs (each optional): feat_nhwc_out (B,h,w,F) dtype;
 * pooled_out (B,F) pooled_dtype (cnn.py:48); ncp_out (B,F,h*w) fp32 (cnn_attn.py:49).
 * train != 0: batch statistics + running-buffer update (main.py:125); else eval mode.
 * train == 2: batch statistics, but the running buffers are left for st_resnet_update_running (same workspace) -- for
 * forwards of successive minibatches that run concurrently on different streams and must apply their momentum updates in order.
 * ---------------------------------------------------------------------------------- */
typedef struct st_resnet st_resnet;
int st_resnet_create(int version, int dtype, st_resnet** out);
void st_resnet_destroy(st_resnet* r);
int st_resnet_num_convs(const st_resnet* r);
int st_resnet_feat_dim(const st_resnet* r);
size_t st_resnet_weight_elems(const st_resnet* r);
size_t st_resnet_bn_channels(const st_resnet* r);
int st_resnet_conv_info(const st_resnet* r, int i, int* cin, int* cout, int* k, int* stride, int* pad,
                        int* cin_padded, size_t* weight_offset, size_t* bn_offset, int* k_order,
                        size_t* frag_weight_offset, int* frag_ntw);
/* frag_ntw > 0: layer i also needs a fragment-major copy of its filters at element offset frag_weight_offset
 * (st_pack_conv_weight_frag(.., ntw = frag_ntw)) for the image-resident kernel; 0: none. */
size_t st_resnet_workspace_bytes(const st_resnet* r, int B, int H, int W);
/* Test / diagnosis aid: with a buffer set, every st_resnet_forward on this handle also copies each residual block's output
 * ([B][h][w][C] in the compute dtype, NHWC) into it, block after block in network order (ResNet-101 @224: 33 blocks, 17.9 MB per
 * image in bf16); buf = NULL switches it off.  The block-by-block parity test feeds these to the oracle one block at a time. */
int st_resnet_set_taps(st_resnet* r, void* buf, size_t bytes);
int st_resnet_forward(const st_resnet* r, const float* images_nchw, int B, int H, int W,
                      const void* weights, const float* bn_gamma, const float* bn_beta,
                      float* bn_running_mean, float* bn_running_var,
                      int train, float momentum, float eps,
                      void* workspace, size_t workspace_bytes,
                      void* feat_nhwc_out, void* pooled_out, int pooled_dtype, float* ncp_out,
                      void* stream);

int st_resnet_update_running(const st_resnet* r, const void* workspace, float* bn_running_mean, float* bn_running_var,
                             float momentum, void* stream);
/* The launch list st_resnet_forward would issue for (B, H, W, train), planned on the host (no device call): one text line per
 * launch, in launch order, the ST_LAYER_LOG format
 *   family,what,cin,cout,k,stride,hin,win,flops,bytes,replicas_out,replicas_in
 * (replicas_out: BatchNorm statistics replicas the launch writes; replicas_in: replicas of the input BatchNorm it reads, 0 without
 * one; bn_reduce_replicas: 1, the replicas it sums).  Returns the text's length and writes it with a terminating NUL when
 * bytes > that length (buf = NULL, bytes = 0 asks for the length); -1 on an error (st_last_error). */
int st_resnet_plan(const st_resnet* r, int B, int H, int W, int train, char* buf, size_t bytes);

int st_cast2d(const void* x, void* y, int from_dtype, int to_dtype, int rows, int cols, int ldx, int ldy, void* stream);

/* ------------------------------------------------------------------------------------
 * Teacher-forced recurrent decoder over a packed sequence.
 * Replaces RNN.forward (rnn.py:27-35; LSTM/rnn_lstm.py:25-33): nn.Embedding + cat +
 * pack_padded_sequence + nn.GRU/nn.LSTM (cuDNN fused RNN) + nn.Linear, and the autograd
 * backward of the same graph (main.py:151).
 * Rows are time-major packed as pack_padded_sequence orders them: row(t,b) = off[t] + b.
 *   rows_b/rows_t: (b, t) of every packed row; prev_row: index of row(t-1,b) (unused for t=0).
 *   batch_sizes_host: HOST array, non-increasing (captions sorted by length, utils.py:66).
 * Weights are [G*H][in] / [G*H][H] in `dtype` (gate order r,z,n / i,f,g,o as torch), biases fp32.
 * The workspace carries the saved activations from st_rnn_forward to st_rnn_backward.
 * st_rnn_forward: logits[ntok][ldl] (optional) and targets[ntok] = caption[b][t] (main.py:145).  in0 must equal E: the layer-0
 *   rows are [feature ; embeddings], gathered by the call.
 * st_rnn_backward: gradients are ACCUMULATED (+=) into the fp32 buffers of st_rnn_grads;
 *   dlogits (required) is [ntok][ldd] in `dtype` with ldd a multiple of 8 and zero pad columns;
 *   dfeat[B][E] (fp32) receives the gradient w.r.t. the image feature rows.
 * Both take the step's dropout (st_dropout below; NULL or every p = 0: none) and input_ids [B][Tcap] int64 on the device
 * (scheduled sampling; NULL = s->caption): the layer-0 rows t >= 1 gather emb[input_ids[b][t-1]], the targets still come from
 * s->caption, and the backward pass scatters the embedding gradient to input_ids.  NULL for either is the plain call, launch
 * for launch.
 * ---------------------------------------------------------------------------------- */
#define ST_MAX_LAYERS 8
typedef struct {
  int cell, dtype, L, in0, H, V, E;
  const void* emb;                                   /* [V][E] dtype                  */
  const void* w_ih[ST_MAX_LAYERS]; const void* w_hh[ST_MAX_LAYERS];
  const float* b_ih[ST_MAX_LAYERS]; const float* b_hh[ST_MAX_LAYERS];
  const void* w_lin; const float* b_lin;             /* [V][H] dtype, [V] fp32        */
} st_rnn_params;

typedef struct {
  float* emb;
  float* w_ih[ST_MAX_LAYERS]; float* w_hh[ST_MAX_LAYERS]; float* b_ih[ST_MAX_LAYERS]; float* b_hh[ST_MAX_LAYERS];
  float* w_lin; float* b_lin;
} st_rnn_grads;

typedef struct {
  int B, T, ntok, Tcap;
  const int* batch_sizes_host;
  const int* rows_b; const int* rows_t; const int* prev_row;   /* device int32 [ntok] */
  const long* caption;                                          /* device int64 [B][Tcap] */
} st_packed_seq;

/* leading dimension (elements) for the logits / dlogits rows of a V-entry vocabulary: up8(V) below 2048 entries, else V
 * rounded up to 512 (the backward product over K = V is then split into 8 even slices); pad columns are zero-filled */
int st_rnn_vocab_ld(int V);
/* st_rnn_workspace_bytes, st_rnn_greedy_workspace_bytes, st_rnn_sample_workspace_bytes, st_rnn_sched_inputs_workspace_bytes and
 * the st_attn_*_workspace_bytes planners return 0 for a descriptor no entry point accepts: a null pointer, a batch below 1, a
 * layer count outside [1, ST_MAX_LAYERS] (the *_dropout_bytes and *_fused_loss*_bytes counts do not look at the layer count) */
size_t st_rnn_workspace_bytes(const st_rnn_params* p, const st_packed_seq* s);

/* ------------------------------------------------------------------------------------
 * Dropout for the teacher-forced decoders: nn.GRU(dropout = p) between layers, nn.Dropout in front of `linear` and on the layer-0
 * input rows.  The kernels hold no generator state.  The mask is a pure function of (seed, step, site, packed row, column)
 * (csrc/dropout.h):  words = Philox4x32-10(counter = (column / 4, packed row, site, step), key = (seed low 32, seed high 32)), word e
 * belongs to column 4 * (column / 4) + e;  an element is kept iff word >= (uint32) floor(p * 2^32);  a kept element is
 * T(float(x) * float(1 / (1 - p))), a dropped one +0.  The packed row is row(t, b) of st_packed_seq, so the mask depends on no launch
 * geometry or route.  Sites: l = the output of recurrent layer l (L - 1: the rows `linear` reads), 255 = the layer-0 input rows.
 *   st_dropout_rows: y[r][c] = masked x[r][c] for r < rows, c < cols (cols, ldx, ldy multiples of 4; fp32 or bf16; y == x allowed);
 *                    row0 is the packed row of x's first row.
 * st_dropout describes one training step's dropout.  Each p is in [0, 1), 0 = that site off.  p_layer applies to the output of every
 * layer but the last (nothing for L = 1).  `buf` (st_rnn_dropout_bytes / st_attn_dropout_bytes; the caller's, needed when p_layer or
 * p_out is on) receives the dropped copies, L matrices [ntok][H] in the compute dtype, and carries them from the forward call to the
 * loss and backward calls of the same step, which take the same descriptor.  The workspaces stay what they are.
 * A NULL descriptor (or every p = 0) is the plain call, launch for launch:
 *   st_rnn_forward:        x0 is masked in place (p_in); with p_layer the wavefront's cells write h' for their recurrence and the
 *                          dropped h' for the layer above, in the same launches; with p_out the projection reads the dropped copy
 *                          of y_top;
 *   st_rnn_fused_loss /    the fused loss and its dlogits read the dropped copy of y_top (p_out);
 *   st_rnn_fused_dlogits:
 *   st_rnn_backward:       dy_top and dx0 are masked (fp32, in place), the fused BPTT cell masks the product it takes from the
 *                          layer above in registers (with p_layer the call is the fused route whatever ST_BPTT_FUSED says),
 *                          dW_ih_{l+1} and dW_lin contract with the dropped copies, dW_hh_l with the plain rows;
 *   st_attn_forward /      p_out only (p_in, p_layer must be 0): the recurrence and the next step's attention read the plain top
 *   st_attn_backward:      state; the projection and dW_lin the dropped copy; dy_top is masked before the step loop.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  double p_in, p_layer, p_out;
  long seed;                                         /* 64 bits, both halves key the generator */
  int step;                                          /* >= 0: one per training step            */
  void* buf; size_t buf_bytes;
} st_dropout;

int st_dropout_rows(const void* x, void* y, int dtype, int rows, int cols, int ldx, int ldy, double p, long seed, int step,
                    int site, int row0, void* stream);
size_t st_rnn_dropout_bytes(const st_rnn_params* p, const st_packed_seq* s);
int st_rnn_forward(const st_rnn_params* p, const st_packed_seq* s, const void* feat,
                   void* workspace, size_t workspace_bytes, void* logits, int logits_dtype, int ldl,
                   long* targets, int save_for_backward, const st_dropout* drop, const long* input_ids, void* stream);
int st_rnn_backward(const st_rnn_params* p, const st_rnn_grads* g, const st_packed_seq* s, const void* dlogits, int ldd,
                    void* workspace, size_t workspace_bytes, float* dfeat, const st_dropout* drop, const long* input_ids,
                    void* stream);

/* The terms of a cross-entropy call beyond the plain mean: per-row weights (reward-weighted training), the per-row losses (scoring
 * of given captions) and label smoothing, torch's nn.CrossEntropyLoss(label_smoothing = eps).  With nll_r = logsumexp(x_r) -
 * x_r[target_r] and u_r = logsumexp(x_r) - (1 / V) * sum_{v < V} x_r[v] (cross entropy against the uniform distribution):
 *   *loss_accum += sum_r row_weight[r] * ((1 - eps) * nll_r + eps * u_r) / rows   (the divisor stays `rows`: row_weight = 1 is the mean);
 *   nll_out[r] = nll_r (unweighted, unsmoothed);  smooth_out[r] = u_r;
 *   dlogits row r = (softmax - (1 - eps) * onehot - eps / V) * row_weight[r] * grad_scale / rows (the weight is a constant of the loss).
 * The buffers are the caller's fp32 device buffers.  A NULL st_loss_terms* is the plain mean cross entropy. */
typedef struct {
  const float* row_weight;   /* [rows] fp32, packed-row order, or NULL (= 1)                          */
  float*       nll_out;      /* [rows] or NULL: the rows' unweighted, unsmoothed -log p(target)       */
  int          smoothing;    /* 0: the kernels without the smoothing term; 1: the label-smoothing
                                kernels, at any label_smoothing in [0, 1) -- 0 then computes what
                                smoothing = 0 computes, bit for bit                                   */
  float        label_smoothing;   /* eps, checked (NaN is refused); must be 0 with smoothing = 0      */
  float*       smooth_out;   /* [rows] or NULL (smoothing = 1 only): logsumexp - mean logit           */
  float*       tile_sums; size_t tile_sums_bytes;   /* fused route with smoothing = 1 only
                                                       (st_rnn_fused_loss_ls_bytes)                   */
} st_loss_terms;

/* Vocabulary projection (rnn.py:33) + nn.CrossEntropyLoss() (main.py:94,149) WITHOUT a logits tensor (csrc/vocab_ce.hip; bf16, H = 512):
 * after st_rnn_forward(.., logits = NULL, .., targets, save_for_backward = 1):
 *   st_rnn_fused_loss:    the loss of st_loss_terms over x = y_top W_lin^T + b_lin computed tile by tile; loss_accum may be NULL when
 *                         nll_out or smooth_out is given.  `scratch` (st_rnn_fused_loss_bytes) keeps the rows' logsumexp for the
 *                         backward call.  With smoothing = 1 the rows' mean logit is formed tile by tile too: `tile_sums`
 *                         (st_rnn_fused_loss_ls_bytes, dead after the call) receives each 128-entry tile's sum per token and is
 *                         added in a fixed order, so u_r is bit-reproducible;
 *   st_rnn_fused_dlogits: dlogits[ntok][ldd] (bf16) with grad_scale = *grad_scale_dev from the same tile products, pad columns
 *                         [V, ldd) exact zeros: the operand st_rnn_backward takes.  Of `terms` it reads row_weight, smoothing and
 *                         label_smoothing.
 * Both read the rows `linear` read: with drop->p_out > 0 the dropped copy of y_top in drop->buf, else the workspace's.
 * Replaces st_rnn_forward's logits + two st_cross_entropy passes (the logits are never written, dlogits once). */
int st_rnn_fused_loss_supported(const st_rnn_params* p);
size_t st_rnn_fused_loss_bytes(const st_rnn_params* p, const st_packed_seq* s);
size_t st_rnn_fused_loss_ls_bytes(const st_rnn_params* p, const st_packed_seq* s);
int st_rnn_fused_loss(const st_rnn_params* p, const st_packed_seq* s, const void* workspace, size_t workspace_bytes,
                      const long* targets, float* scratch, size_t scratch_bytes, const st_loss_terms* terms, float* loss_accum,
                      const st_dropout* drop, void* stream);
int st_rnn_fused_dlogits(const st_rnn_params* p, const st_packed_seq* s, const void* workspace, size_t workspace_bytes,
                         const long* targets, const float* scratch, const float* grad_scale_dev, const st_loss_terms* terms,
                         void* dlogits, int ldd, const st_dropout* drop, void* stream);

/* nn.CrossEntropyLoss() forward + backward (main.py:94,149) on logits rows, with the terms of st_loss_terms (NULL: the plain mean;
 * tile_sums is not read).  dlogits may alias logits when the dtypes match; pad columns [V, ldd) are zero-filled. */
int st_cross_entropy(const void* logits, int logits_dtype, const long* target, int rows, int V, int ldl,
                     const st_loss_terms* terms, float* loss_accum, void* dlogits, int dlogits_dtype, int ldd, float grad_scale,
                     const float* grad_scale_dev /* optional device scalar multiplied in */, void* stream);

/* Encoder head: y = BatchNorm1d(x W^T + b) (cnn.py:37-38,49; momentum 0.01) and its backward
 * (dx is not needed: the backbone output is detached, cnn.py:47).  Gradients are accumulated. */
size_t st_head_workspace_bytes(int B, int F, int E, int dtype);
int st_linear_bn1d_forward(const void* x, const void* w, const float* bias, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, int B, int F, int E, int dtype,
                           int train, float momentum, float eps,
                           float* z_out, float* save_mean, float* save_rstd, void* y_dtype, float* y_f32, void* stream);
int st_linear_bn1d_backward(const float* dy, const float* z, const void* x, const float* gamma,
                            const float* save_mean, const float* save_rstd, int B, int F, int E, int dtype, int train,
                            float* dw, float* dbias, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                            void* stream);

/* torch.optim.SGD(lr, momentum) / torch.optim.Adam(lr) (main.py:97-100,152) over one flat fp32
 * buffer; bf16_shadow (optional) receives the updated parameters rounded to bf16. */
int st_sgd_step(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, long n,
                float lr, float momentum, int first_step, float grad_scale, void* stream);
int st_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow, long n,
                 float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream);

/* Global-norm gradient clipping, weight decay and a non-finite guard for the two optimizers, with nothing read back by the host.
 * st_grad_sumsq writes one partial sum of squares of grad[0..n) per workgroup into `partials` (device, room for
 * st_grad_sumsq_max_parts() floats) and the number written into *nparts_out (host); the grid depends on n only and no float
 * atomics are used, so the same input gives the same bits.  The _ex steps, launched after it on the same stream, add the
 * partials up in every workgroup (fixed order) and derive
 *     norm = grad_scale * sqrt(sum)                       (flat_grad holds the sum over ranks, grad_scale = 1 / world)
 *     coef = grad_scale * min(1, max_norm / (norm + 1e-6))    (torch.nn.utils.clip_grad_norm_; max_norm <= 0: coef = grad_scale)
 * then  g' = coef * g + weight_decay * p  (SGD; Adam with decoupled = 0, as torch.optim.Adam(weight_decay=)), or
 * p *= 1 - lr * weight_decay and the moments from coef * g  (decoupled = 1, torch.optim.AdamW).
 * skip_nonfinite: a launch whose sum is not finite leaves param, the state and the shadow untouched and counts as skipped;
 * Adam's bias correction (and SGD's "first step") then follow the count of APPLIED steps kept in `status` instead of
 * `step` / `first_step`.  Without it a non-finite norm propagates as torch's does.
 * status: ST_OPTIM_STATUS_WORDS 32-bit words of device memory owned by the caller, zeroed (or set to a restored step count in
 * words 2, 4, 5) before the first call:  [0] float last norm, [1] float last coef, [2] int applied steps, [3] int skipped steps,
 * [4], [5] int the applied count as two slots.  A launch reads slot `parity` and writes slot `parity ^ 1`: the caller passes
 * 0, 1, 0, 1, .. on consecutive _ex calls that share a status block. */
#define ST_OPTIM_STATUS_WORDS 8
int st_grad_sumsq_max_parts(void);
int st_grad_sumsq(const float* grad, long n, float* partials, int* nparts_out, void* stream);
int st_sgd_step_ex(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, long n,
                   float lr, float momentum, int first_step, float grad_scale, const float* partials, int nparts,
                   float max_norm, float weight_decay, int skip_nonfinite, int parity, void* status, void* stream);
int st_adam_step_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow, long n,
                    float lr, float beta1, float beta2, float eps, int step, float grad_scale, const float* partials,
                    int nparts, float max_norm, float weight_decay, int decoupled, int skip_nonfinite, int parity,
                    void* status, void* stream);

/* Greedy decoding, exactly `steps` iterations with no early stop (rnn.py:37-58, rnn_lstm.py:35-57):
 * ids_out[B][steps] int64 (first-maximum tie rule of torch.max).  logits_out (optional, tests):
 * [steps][B][Vp] fp32 with Vp = V rounded up to 8. */
size_t st_rnn_greedy_workspace_bytes(const st_rnn_params* p, int B);
int st_rnn_greedy(const st_rnn_params* p, const void* feat, int B, int steps, void* workspace, size_t workspace_bytes,
                  long* ids_out, float* logits_out, void* stream);
/* Which route the calling thread's last st_rnn_greedy took: 0 = the pipelined decoder (csrc/decode_pipe.hip) ran;
 * 1 = the launch chain, because the call is not eligible for the pipe (configuration, logits_out, steps, stream capture,
 * ST_DECODE_PIPE=0); 2 = the launch chain after the pipe gave up (no co-resident grid, uneven XCD placement, CU count). */
int st_rnn_greedy_last_route(void);

/* Building blocks of the beam decoders (rnn.py:60-108 and beam_search.py:45-97):
 * st_rnn_step: one timestep of the L-layer cell for n independent rows, states [L][n][H] in `dtype`
 *   (h_in/c_in NULL = zero state, as nn.GRU(x, None)), optional fp32 logits [n][ldl] = linear(h_top);
 * st_embedding_rows: x[r] = embeddings[ids[r]] (rnn.py:53,85);
 * st_gather_state: dst[l][r] = src[l][idx[r]] (a child beam inherits its parent's recurrent state);
 * st_softmax_topk: per row the k largest entries in DESCENDING order with their indices; values are
 *   softmax probabilities (beam_search.py:83-88) or, with raw != 0, the raw logits (rnn.py:90-91). */
int st_rnn_step(const st_rnn_params* p, const void* x, int n, const void* h_in, const void* c_in,
                void* h_out, void* c_out, float* logits, int ldl, void* stream);
int st_embedding_rows(const void* emb, const long* ids, void* out, int n, int E, int V, int ldo, int dtype, void* stream);
int st_gather_state(const void* src, const int* idx, void* dst, int L, int n_src, int n_dst, int H, int dtype, void* stream);
int st_softmax_topk(const float* logits, int ldl, int n, int V, int k, float* top_p, long* top_id, int raw, void* stream);
/* st_beam_ban_topk: st_softmax_topk (probabilities) with a per-row ban set, the top-k launch of a beam iteration that has
 *   something to ban.  Entry v of a row is banned iff it is one of the n_suppress ids of `suppress` (device memory; ids
 *   outside [0, V) are ignored), or v == end_id and ban_end != 0 (the host's "fewer than min_length words so far"), or
 *   ngram = g >= 1 and appending v to the row's path s_0 .. s_t (hist [n][hist_ld] int32, t = hist_len - 1, s_0 = <start>;
 *   NULL allowed with g == 0) would repeat an n-gram of size g already on it:
 *   s[i .. i+g-2] == s[t-g+2 .. t] and s[i+g-1] == v for some 0 <= i <= t-g+1 (g == 1 bans every token of the path).
 *   The softmax still runs over all V entries, so a probability is the model's own; the k results are the k most probable
 *   unbanned entries (lowest index first among equals), and a row with fewer than k of them ends in (p = 0, id = 0) entries.
 *   With an empty ban set the outputs are st_softmax_topk's, bit for bit. */
#define ST_BEAM_MAX_NGRAM 16
#define ST_BEAM_MAX_SUPPRESS 64
#define ST_BEAM_MAX_HIST 64          /* tokens of a path, <start> included: max_length + 1 */
#define ST_BEAM_MAX_VOCAB 524288     /* bits of the ban map (64 KB of LDS) */
int st_beam_ban_topk(const float* logits, int ldl, int n, int V, int k, const int* hist, int hist_ld, int hist_len, int ngram,
                     const long* suppress, int n_suppress, long end_id, int ban_end, float* top_p, long* top_id, void* stream);
/* One iteration of beam_search.py:69-94 for B images on the device, the one fringe selection of every beam search: fringe slots
 * (b, w), w < W, hold (tok, cost) with cost = +inf for an empty slot; top_p/top_id are the top-k launch's rows of the B*W slots
 * (k entries, descending).  Writes the new fringe (stable W-best of the node-major, ascending-probability candidate list by
 * float32 cumulative -log p), every new node's parent slot (-1: empty), ended[b][w] = old slot held <end> (to be harvested),
 * gather[b*W+w] = state row of the parent, and updates done (no live node left).
 * Paths: hist_in and hist_out are both NULL (no paths kept) or two different buffers [B*W][hist_ld] int32, and every new node is
 * handed its path: hist_out[b*W + rank] = hist_in[b*W + parent][0 .. hist_len) followed by the node's token (zeros for an empty
 * slot); 1 <= hist_len and hist_len + 1 <= min(hist_ld, ST_BEAM_MAX_HIST).
 * Groups (diverse beam search, Vijayakumar et al., AAAI 2018): the W slots are G groups of W' = W / G slots, group g = slots
 * g*W' .. (g+1)*W' - 1; G = 1 with diversity_penalty = 0 is the single beam.  Each group is a search of its own: done [B][G],
 * harvest flags per group, and a parent (an image-wide slot index) always lies in its child's group.  The groups of an image are
 * handled in the order 0 .. G-1 inside the one launch.  A candidate of group g (its W' nodes x their k list entries, node-major,
 * ascending probability) has raw = fl32(cost[w] + fl32(-log(double p))) and key = fl32(raw + fl32(diversity_penalty * n_v)),
 * n_v = the number of occupied slots of the new fringes of groups 0 .. g-1 that hold the candidate's word (a count; <end> counts
 * like any word); raw = +inf stays +inf.  The group's new fringe is its W' best by a stable ranking of key, in rank order;
 * new_cost records raw, never the penalty.
 * Needs G >= 1, W % G == 0, a finite diversity_penalty >= 0, k <= W and W * k <= 64. */
int st_beam_select(const long* tok, const float* cost, uint8_t* done, const float* top_p, const long* top_id, int B, int W, int G,
                   int k, long end_id, float diversity_penalty, long* new_tok, float* new_cost, int* parent, uint8_t* ended,
                   int* gather, const int* hist_in, int* hist_out, int hist_ld, int hist_len, void* stream);

/* Caption sampling (the multinomial counterpart of the max(1)[1] of rnn.py:52 and rnn_attn.py:141).  The kernels hold no
 * random-number generator: the caller supplies one uniform in [0, 1) per row and step.
 * st_sample_rows: for n rows of fp32 logits [n][ldl] (V valid entries, as st_rnn_step writes them) draw one token per row from
 *   u[r * u_stride].  With z_v = logits[v] * inv_temperature (inv_temperature > 0) the kept set K is every v < V (top_k == 0)
 *   or exactly the indices st_softmax_topk returns for the row (1 <= top_k <= min(32, V): the largest logits, the lowest index
 *   first among equal values); p_v = exp(z_v - max_K z) / sum_K exp(z - max_K z); the token is the smallest v of K, in index
 *   order, whose inclusive cumulative probability over K exceeds u (the largest v of K if rounding leaves none);
 *   logp = z_tok - max - log(sum), the log-probability under the distribution sampled from (0 with top_k == 1).
 *   A row needs at least one finite entry (st_rnn_step's logits have): with none the token is 0 and logp is NaN.
 *   finished[n] (bytes, read and written): a row finished on entry gets token 0 (<pad>) and logp 0 and stays finished, a row
 *   that draws end_id is marked finished after the draw.  The token goes to ids_out[r * out_stride + t] and to cur[r] (the
 *   buffer the next st_embedding_rows reads; nullable), logp to logp_out[r * out_stride + t].
 * st_rnn_sample: the loop of rnn.py:37-58 with the draw in place of max(1)[1]: step 0 feeds feat [n][E] (dtype) from a zero
 *   state, each later step the embedding of the row's last token, exactly `steps` iterations of st_rnn_step (with logits),
 *   st_sample_rows, st_embedding_rows.  u [n][steps] fp32; ids_out [n][steps] int64 and logp_out [n][steps] fp32.
 * Nothing is allocated or synchronised inside these calls. */
int st_sample_rows(const float* logits, int ldl, int n, int V, const float* u, int u_stride, float inv_temperature, int top_k,
                   long end_id, uint8_t* finished, long* ids_out, float* logp_out, int out_stride, int t, long* cur, void* stream);
size_t st_rnn_sample_workspace_bytes(const st_rnn_params* p, int n);
int st_rnn_sample(const st_rnn_params* p, const void* feat, int n, int steps, const float* u, float inv_temperature, int top_k,
                  long end_id, void* workspace, size_t workspace_bytes, long* ids_out, float* logp_out, void* stream);
/* Nucleus (top-p) sampling (Holtzman et al., 2020): the siblings above with one more filter, 0 < top_p <= 1 (anything else,
 * NaN included, is refused before a launch).  Order of the filters: temperature, top_k, top_p.  Order the entries of K (above)
 * by value descending, the lowest index first among equal values (+0.0 and -0.0 are equal); entry j is kept iff the
 * probability mass, renormalised over K, of the entries strictly before it is below top_p.  The first entry is always kept,
 * entries of weight 0 (-inf) come last, and the nucleus may be any size from 1 to V.  The token is drawn among the kept
 * entries in index order from u as above, and logp is its log-probability under the kept, renormalised distribution.
 * top_p = 1 is the filter OFF, not a nucleus of mass 1: the call is then its sibling's, the same launch bit for bit (the
 * siblings forward here with top_p = 1).  The draw is a pure function of (logits, u, inv_temperature, top_k, top_p): no
 * floating-point atomics, every sum in a fixed order.  Same workspaces, same single launch per step. */
int st_sample_rows_topp(const float* logits, int ldl, int n, int V, const float* u, int u_stride, float inv_temperature, int top_k,
                        float top_p, long end_id, uint8_t* finished, long* ids_out, float* logp_out, int out_stride, int t, long* cur,
                        void* stream);
int st_rnn_sample_topp(const st_rnn_params* p, const void* feat, int n, int steps, const float* u, float inv_temperature, int top_k,
                       float top_p, long end_id, void* workspace, size_t workspace_bytes, long* ids_out, float* logp_out, void* stream);
/* Scheduled sampling (Bengio et al., 2015): the inputs of a teacher-forced pass with some slots holding the model's own draw.
 * st_sample_mix_rows: st_sample_rows' draw (same rule, same routes, same u) and the mix in one launch, without a finished state
 *   (the caption decides a row's length).  Row r is REPLACED iff step < lens[r] and coin[r * coin_stride] < p (strict: p = 0
 *   replaces nothing, p = 1 every valid row; a NaN coin never): the drawn token goes to mixed_out[r * out_stride + t], to cur[r]
 *   and to ids_out[r * out_stride + t], its log-probability to logp_out, and replaced_out[r * out_stride + t] = 1.  Every other
 *   row skips the draw: the teacher's token teacher[r * teacher_stride + teacher_col] goes to mixed_out and cur, replaced_out = 0,
 *   ids_out = -1, logp_out = 0.  `step` is the step the slot feeds, lens [n] int32 on the device; ids_out / logp_out may be NULL.
 * st_rnn_sched_inputs: the loop of st_rnn_sample following the caption [n][Tcap] instead of free-running, all n rows for
 *   max_len - 1 steps (max_len = max(lens), given by the caller: nothing is read back): step t's logits decide slot t, which
 *   feeds step t + 1 and is valid iff t + 1 < lens[r].  coin, u [n][Tcap] fp32.  Outputs, all [n][Tcap] and written in full:
 *   input_ids (int64; the caption wherever replaced is 0), replaced (bytes), and optionally (NULL: not wanted) drawn (int64, the
 *   drawn token, -1 where not replaced) and logp (fp32, its log-probability, 0 where not replaced).  Workspace: that of
 *   st_rnn_sample.  Never any dropout: the roll-in runs the deterministic model, as st_rnn_sample does.
 * Nothing is allocated or synchronised inside these calls. */
int st_sample_mix_rows(const float* logits, int ldl, int n, int V, const float* u, int u_stride, float inv_temperature, int top_k,
                       const float* coin, int coin_stride, float p, const long* teacher, int teacher_stride, long teacher_col,
                       const int* lens, int step, long* ids_out, float* logp_out, long* mixed_out, uint8_t* replaced_out,
                       int out_stride, int t, long* cur, void* stream);
size_t st_rnn_sched_inputs_workspace_bytes(const st_rnn_params* p, int n);
int st_rnn_sched_inputs(const st_rnn_params* p, const void* feat, int n, const long* caption, int Tcap, const int* lens, int max_len,
                        const float* coin, const float* u, float prob, float inv_temperature, int top_k, void* workspace,
                        size_t workspace_bytes, long* input_ids, uint8_t* replaced, long* drawn, float* logp, void* stream);

/* CIDEr rewards of sampled captions (self-critical training), the score of evaluation.cider_score in one launch, one workgroup per
 * image.  A caption's words are its ids before the first end_id, within its length.  An n-gram (n = 1 .. 4) is ONE 64-bit key, packed
 * exactly: token j contributes (id + 1) << (16 * j), ids in [0, 65534]; the highest non-zero field gives the order.
 *   table      keys [K] int64 sorted ascending AS SIGNED, strictly; df [K] int32 with 1 <= df <= num_docs; log_num_docs =
 *              log(num_docs) >= 0.  An n-gram the table lacks has df 0, so its idf is log_num_docs.
 *   references refs [B][R][Tr] int32 words only (the caller has cut them at end_id), ref_len [B][R] int32 words per row,
 *              ref_count [B] int32 rows of image b in use (the score divides by it; 0 gives a score of 0).
 *   candidates ids [B][S][T] int64 and lengths [B][S] int64 exactly as st_rnn_sample / sample_lengths leave them; greedy_ids
 *              [B][Tg] int64 or NULL (its length is Tg).
 *   weight of an n-gram g: w = tf * (log_num_docs - log(max(1, df(g)))); norm_n = sqrt(sum over distinct g of w^2); per candidate,
 *   reference and order val_n = sum over the candidate's distinct g of min(w_c, w_r) * w_r, divided by norm_c * norm_r when both are
 *   non-zero, times exp(-(len_c - len_r)^2 / (2 sigma^2)), len = max(words - 1, 0); score = 10 * mean_n(sum_refs val_n) / ref_count.
 *   outputs    score64 [B][S + 1] float64 (column S is the greedy caption's and is written only when greedy_ids is given),
 *              reward [B][S] fp32 = score64 rounded, advantage [B][S] fp32 (baseline 1: reward - greedy reward; 2: reward - the
 *              mean of the image's OTHER rewards; formed from the fp32 rewards in double and rounded once, as
 *              train.self_critical_advantage; baseline 0: not written, may be NULL).
 * Refused before the launch, outputs untouched: R outside [1, ST_CIDER_MAX_REFS], Tr, T or Tg outside [1, ST_CIDER_MAX_TOKENS],
 * S < 1, baseline outside 0 .. 2, baseline 2 with S < 2, baseline 1 without greedy_ids, sigma <= 0, log_num_docs < 0, end_id outside
 * [0, 65534].  What lives in device memory cannot be refused here without a round trip: lengths, ref_len and ref_count are CLAMPED
 * to their rows (the Python callers refuse lengths > T), and a sampled id outside [0, 65534] is taken as impossible and not
 * checked -- st_rnn_sample draws ids below V, and a vocabulary that large is refused when the references are packed; such an id
 * would alias another word (16 bits are kept), never touch memory out of bounds.
 * float64 on the vector ALU throughout; every sum in a fixed order, no floating-point atomics, no workspace: two identical captions
 * score bit-identically.  Nothing is allocated or synchronised inside the call. */
#define ST_CIDER_MAX_REFS 8
#define ST_CIDER_MAX_TOKENS 64
int st_cider_reward(const long* keys, const int* df, long K, double log_num_docs, const int* refs, const int* ref_len,
                    const int* ref_count, int B, int R, int Tr, const long* ids, const long* lengths, int S, int T,
                    const long* greedy_ids, int Tg, long end_id, double sigma, int baseline, double* score64, float* reward,
                    float* advantage, void* stream);

/* ------------------------------------------------------------------------------------
 * Soft-attention decoder (Attention/rnn_attn.py, rnn_attn_LSTM.py; train step Attention/main_attn.py:123-134).
 *   features: cnn_feature (B,F,P) fp32 as cnn_attn.py:49 returns it; caption_T: int64 [Tcap][B] (transposed captions).
 *   Per step t (rnn_attn.py:66-74): attention over P pixels keyed on the last layer's h, x = [emb(cap[:,t]) ; embed(z)],
 *   one step of the L-layer cell on the first B_t rows, logits rows written time-major packed (rnn_attn.py:115).
 *   alphas (B,T,P) fp32 must be zero-filled by the caller (the reference zero-pads, rnn_attn.py:65).
 *   The time-invariant encoder_att projection is computed once per batch instead of once per step.
 * st_attn_backward accumulates (+=) every parameter gradient, including the doubly-stochastic term
 *   alpha_c * mean((1 - sum_t alpha)^2) (main_attn.py:131) scaled like the loss (grad_scale_dev, optional).
 * st_attn_reg_loss adds that term to *loss_accum.
 * ---------------------------------------------------------------------------------- */
typedef struct {
  st_rnn_params rnn;                               /* rnn.in0 = 2E */
  int F, A, P;
  const void* w_enc; const float* b_enc;           /* attn.encoder_att [A][F] dtype, [A] */
  const void* w_dec; const float* b_dec;           /* attn.decoder_att [A][H] dtype, [A] */
  const float* w_full; const float* b_full;        /* attn.full_att    [A] fp32, [1]     */
  const void* w_init_h; const float* b_init_h;     /* init_h [H][F] dtype                */
  const void* w_init_c; const float* b_init_c;     /* init_c (LSTM only)                 */
  const void* w_embed; const float* b_embed;       /* embed [E][F] dtype                 */
} st_attn_params;

typedef struct {
  st_rnn_grads rnn;
  float *w_enc, *b_enc, *w_dec, *b_dec, *w_full, *b_full, *w_init_h, *b_init_h, *w_init_c, *b_init_c, *w_embed, *b_embed;
} st_attn_grads;

size_t st_attn_workspace_bytes(const st_attn_params* p, const st_packed_seq* s);
/* `drop`: Dropout in front of `linear` (st_dropout above: p_out only; NULL = none) */
size_t st_attn_dropout_bytes(const st_attn_params* p, const st_packed_seq* s);
int st_attn_forward(const st_attn_params* p, const st_packed_seq* s, const float* cnn_feature, const long* caption_T,
                    void* workspace, size_t workspace_bytes, void* logits, int logits_dtype, int ldl,
                    float* alphas, int save_for_backward, const st_dropout* drop, void* stream);
int st_attn_backward(const st_attn_params* p, const st_attn_grads* g, const st_packed_seq* s, const long* caption_T,
                     const void* dlogits, int ldd, const float* alphas,
                     const float* dalphas /* (B,T,P) gradient w.r.t. alphas from the caller, or NULL: use alpha_c */,
                     float alpha_c, const float* grad_scale_dev, void* workspace, size_t workspace_bytes, const st_dropout* drop,
                     void* stream);
int st_attn_reg_loss(const float* alphas, int B, int T, int P, float alpha_c, float* loss_accum, void* stream);
/* rnn_attn.py:120-145 (test branch 77-94): `steps` greedy iterations from <start>; ids_out[B][steps] int64 */
size_t st_attn_greedy_workspace_bytes(const st_attn_params* p, int B);
int st_attn_greedy(const st_attn_params* p, const float* cnn_feature, int B, int steps, long start_id,
                   void* workspace, size_t workspace_bytes, long* ids_out, void* stream);
/* st_attn_greedy plus the attention map of every step: alphas_out[B][steps][P] fp32 (same workspace as st_attn_greedy) */
int st_attn_greedy_alphas(const st_attn_params* p, const float* cnn_feature, int B, int steps, long start_id,
                          void* workspace, size_t workspace_bytes, long* ids_out, float* alphas_out, void* stream);
/* The same loop (rnn_attn.py:120-145, test branch 77-94) with st_sample_rows in place of the arg-max of rnn_attn.py:141:
 * n rows, u [n][steps] fp32 uniforms, ids_out [n][steps] int64, logp_out [n][steps] fp32, alphas_out [n][steps][P] fp32 or NULL. */
size_t st_attn_sample_workspace_bytes(const st_attn_params* p, int n);
int st_attn_sample(const st_attn_params* p, const float* cnn_feature, int n, int steps, long start_id, const float* u,
                   float inv_temperature, int top_k, long end_id, void* workspace, size_t workspace_bytes,
                   long* ids_out, float* logp_out, float* alphas_out, void* stream);
/* st_attn_sample with the nucleus filter of st_sample_rows_topp (0 < top_p <= 1; top_p = 1 is st_attn_sample itself) */
int st_attn_sample_topp(const st_attn_params* p, const float* cnn_feature, int n, int steps, long start_id, const float* u,
                        float inv_temperature, int top_k, float top_p, long end_id, void* workspace, size_t workspace_bytes,
                        long* ids_out, float* logp_out, float* alphas_out, void* stream);
/* st_rnn_sched_inputs for the attention decoders (the loop of st_attn_sample following the caption): step t feeds slot t, so
 * step t's logits decide slot t + 1, valid iff t + 1 < lens[r]; slot 0 (<start>) is never replaced.  caption [n][Tcap] and its
 * transpose caption_T [Tcap][n] (what st_attn_forward takes); coin, u and the outputs as st_rnn_sched_inputs. */
size_t st_attn_sched_inputs_workspace_bytes(const st_attn_params* p, int n);
int st_attn_sched_inputs(const st_attn_params* p, const float* cnn_feature, int n, const long* caption, const long* caption_T, int Tcap,
                         const int* lens, int max_len, const float* coin, const float* u, float prob, float inv_temperature, int top_k,
                         void* workspace, size_t workspace_bytes, long* input_ids, uint8_t* replaced, long* drawn, float* logp,
                         void* stream);
/* beam_search.py:45-97 on the attention decoder for B images, W slots each (1 <= W <= 8, so W*min(W,V) <= 64): initial state
 * h0 = init_h(mean_p feat) (and c0) over all layers, generate = one test-branch step (rnn_attn.py:77-94) from the node's token.
 * Rows are fixed (image, slot) pairs b*W + w.  Records use beam.py's layout: rec_tok/rec_cost/rec_par [max_length+1][B][W]
 * (fringe after each iteration; slot 0 of fringe 0 is start_id at cost 0), rec_end [max_length][B][W] (harvest flags),
 * rec_alpha [max_length][B*W][P] fp32 (nullable): the attention map of every row at every iteration, so the extras of node
 * (t >= 1, w) are rec_alpha[t-1][b*W + rec_par[t][b][w]].  The whole search in one call; nothing synchronised inside.
 *
 * opts (NULL: the plain search -- one group, nothing banned, no paths kept):
 *   min_length, ngram, suppress, n_suppress: st_beam_ban_topk's rules.  <end> is banned while a node has generated fewer than
 *     min_length words (iteration t < min_length), ngram = no-repeat n-gram size (0: off, at most ST_BEAM_MAX_NGRAM; needs
 *     keep_paths), suppress = n_suppress <= ST_BEAM_MAX_SUPPRESS ids in DEVICE memory that never appear.  The ids cannot be
 *     checked here without a device round trip: ids outside [0, V) are ignored (the Python callers reject them before the call).
 *     The top-k launch of an iteration is st_beam_ban_topk iff there is something to ban (min_length > 0 || ngram > 0 ||
 *     n_suppress > 0; then V <= ST_BEAM_MAX_VOCAB), st_softmax_topk otherwise -- the same bits, and no launch more either way.
 *   keep_paths != 0: every node carries its path through st_beam_select (needs max_length + 1 <= ST_BEAM_MAX_HIST).
 *   num_groups, diversity_penalty: diverse beam search by st_beam_select's rule over num_groups groups of W / num_groups slots
 *     (W % num_groups == 0, diversity_penalty finite and >= 0).  Fringe 0 holds start_id at cost 0 in the first slot of every
 *     group.  The records keep their layout; rec_par holds image-wide slot indices, which lie in the child's group.
 * Workspace: the plain plan; with keep_paths followed by the two path buffers [B*W][max_length + 1] int32, each padded to a
 * multiple of 256 bytes (iteration t reads buffer t & 1 and writes the other, so buffer max_length & 1 holds the paths of the
 * last fringe on return); for num_groups > 1 followed by the B * num_groups done flags.  st_attn_beam_workspace_bytes returns
 * the size (0 where the layout is undefined: bad B, W, max_length or layer count, num_groups that does not divide W, keep_paths with
 * max_length + 1 > ST_BEAM_MAX_HIST; the search checks the other options itself) and, through the nullable last_paths_offset, the byte offset of path buffer
 * max_length & 1 (0 when no paths are kept). */
typedef struct { int min_length, ngram; const long* suppress; int n_suppress;
                 int keep_paths; int num_groups; float diversity_penalty; } st_beam_opts;
size_t st_attn_beam_workspace_bytes(const st_attn_params* p, int B, int W, int max_length, const st_beam_opts* opts,
                                    size_t* last_paths_offset);
int st_attn_beam_search(const st_attn_params* p, const float* cnn_feature, int B, int W, int max_length,
                        long start_id, long end_id, void* workspace, size_t workspace_bytes,
                        long* rec_tok, float* rec_cost, int* rec_par, uint8_t* rec_end, float* rec_alpha,
                        const st_beam_opts* opts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
