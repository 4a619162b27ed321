/* include/avx.h -- C ABI of libavx.so: the MI355X (gfx950) per-frame animal-vision hot path.
 *
 * This is the drop-in boundary.  The reference (Kyaw-Thiha/animal-vision) is pure
 * Python and has no FFI of its own; the entry points below are what a ctypes binding added to the
 * reference's shared helpers would call instead of their NumPy/OpenCV bodies.  Each entry point
 * cites the reference interface it replaces (paths relative to the reference repo).  The
 * reference-side stubs are shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 (AVX_OK) or a negative avx_status; nothing throws across the ABI;
 *     avx_last_error(ctx) returns a human-readable message for the last failure on that ctx;
 *   - an avx_ctx is bound to ONE device and is single-threaded (one caller at a time), matching the
 *     reference's one-frame-in-flight loop (main.py:60-72);
 *   - `stream` is a hipStream_t passed as void*, with HIP's own meaning: NULL is the null (default) stream,
 *     a torch.cuda.Stream.cuda_stream value is accepted as is; every launch is asynchronous on it, with ONE exception:
 *     the first avx_dichromat_u8 call for a (kernel configuration, batch, frame size) that is not in the seeded table
 *     times its candidate launch geometries on the caller's frames (~40 ms, blocking; the results are the same for every
 *     candidate) and remembers the winner in the ctx (the ~38 most recently measured shapes next to the seeded ones; an
 *     older shape is measured again when it returns) -- AVX_MARCH_CHUNKS / AVX_MARCH_NG pin a geometry and skip it;
 *   - frame/plane pointers are DEVICE pointers unless the parameter name ends in `_host`;
 *     the caller owns them; ctx owns only its scratch and its constant tables;
 *   - images are C-contiguous HWC (H x W x 3), batches are N such frames back to back.
 */
#ifndef AVX_H
#define AVX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVX_ABI_VERSION 1

typedef struct avx_ctx avx_ctx;

typedef enum avx_status {
    AVX_OK = 0,
    AVX_ERR_INVALID = -1,     /* bad argument (shape, mode, NULL pointer) */
    AVX_ERR_NO_DEVICE = -2,   /* no HIP device / device index out of range */
    AVX_ERR_HIP = -3,         /* a HIP runtime call failed; see avx_last_error */
    AVX_ERR_UNSUPPORTED = -4, /* valid request this build does not implement */
    AVX_ERR_NOMEM = -5
} avx_status;

/* ---- context, memory, streams ---------------------------------------------------------------- */
int avx_abi_version(void);
int avx_device_count(void);                       /* 0 when no GPU is visible; never fails        */
int avx_init(int device, avx_ctx** out_ctx);      /* AVX_ERR_NO_DEVICE when there is no such GPU  */
void avx_destroy(avx_ctx* ctx);
const char* avx_last_error(const avx_ctx* ctx);   /* ctx may be NULL: message of the last failed avx_init */

int avx_malloc(avx_ctx* ctx, size_t bytes, void** out_dptr);
int avx_free(avx_ctx* ctx, void* dptr);
int avx_host_alloc(avx_ctx* ctx, size_t bytes, void** out_hptr); /* pinned host memory */
int avx_host_free(avx_ctx* ctx, void* hptr);
int avx_memcpy_h2d(avx_ctx* ctx, void* dst, const void* src_host, size_t bytes, void* stream);
int avx_memcpy_d2h(avx_ctx* ctx, void* dst_host, const void* src, size_t bytes, void* stream);
int avx_memcpy_d2d(avx_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream); /* device to device, asynchronous on stream */
int avx_memset(avx_ctx* ctx, void* dst, int value, size_t bytes, void* stream);
int avx_stream_create(avx_ctx* ctx, void** out_stream);
int avx_stream_destroy(avx_ctx* ctx, void* stream);
int avx_sync(avx_ctx* ctx, void* stream);         /* hipStreamSynchronize(stream) */
int avx_stream_wait(avx_ctx* ctx, void* waiter, void* signaler); /* device-side: waiter waits for signaler's work so far */
int avx_device_sync(avx_ctx* ctx);                /* hipDeviceSynchronize() */

/* HIP-event stopwatch ON `stream` (bench.py roofline leg: per-launch duration of the hot kernel). */
int avx_timer_start(avx_ctx* ctx, void* stream);
int avx_timer_stop(avx_ctx* ctx, void* stream, float* out_ms); /* records, synchronises, returns ms */

/* ---- dichromat path: animals/animal_utils.py + animals/<species>.py template -------------------
 *
 * One fused launch replaces, for N uint8 frames,
 *   get_normalized_image   animals/animal_utils.py:41-50   (uint8 -> f32, data-dependent /255)
 *   srgb_to_linear         animals/animal_utils.py:5-11    (256-entry table of the reference's values)
 *   pixels @ T.T           animals/dog.py:43-48            (FMA chain, f32)          [AVX_COLOR_MATRIX]
 *     or sRGB_to_LMS / L-M merge / LMS_to_RGB   animals/cat.py:95-101  (f64 tail)   [AVX_COLOR_CAT_MERGE]
 *   apply_acuity_blur      animals/animal_utils.py:121-145 (cv2.GaussianBlur semantics)   [AVX_POST_GAUSS]
 *     or apply_s_cone_vertical_gain  animal_utils.py:206-259 (per-row blue gain)          [AVX_POST_ROWGAIN]
 *     or apply_anisotropic_acuity_blur_with_streak  animal_utils.py:147-172 (as coded, Q3) [AVX_POST_STREAK]
 *   apply_chroma_compression  animal_utils.py:174-181 (optional)
 *   clip -> linear_to_srgb -> clip -> (x*255+0.5).astype(uint8)   animals/dog.py:54-57
 * Results are bit-identical to the reference executed in the build container (tests/golden). */
enum { AVX_COLOR_MATRIX = 0, AVX_COLOR_CAT_MERGE = 1 };
enum { AVX_POST_NONE = 0, AVX_POST_GAUSS = 1, AVX_POST_ROWGAIN = 2, AVX_POST_STREAK = 3 };

typedef struct avx_dichromat_desc {
    uint32_t struct_size;      /* sizeof(avx_dichromat_desc), for ABI growth                         */
    int32_t color_mode;        /* AVX_COLOR_*                                                        */
    float matrix[9];           /* AVX_COLOR_MATRIX: T row-major, out_i = sum_j T[i][j]*in_j (Q1)      */
    float cat_alpha;           /* AVX_COLOR_CAT_MERGE: LM = alpha*L + beta*M  (cat.py:98-99), both as   */
    float cat_beta;            /*   float32: alpha = f32(a), beta = f32(1.0 - a) computed in double     */
    int32_t post_mode;         /* AVX_POST_*                                                         */
    int32_t ksize;             /* AVX_POST_GAUSS: odd tap count (same in x and y), 1..AVX_MAX_KSIZE   */
    const double* taps_host;   /* AVX_POST_GAUSS: ksize normalised taps in double (getGaussianKernel);
                                  the library rounds them to the compute type (f32, or f64 for cat)  */
    const float* row_gain_host;/* AVX_POST_ROWGAIN: H per-row gains for channel 2 (host pointer)      */
    int32_t row_gain_clamp;    /* AVX_POST_ROWGAIN: clip channel 2 to [0,1] after the gain            */
    int32_t chroma_enable;     /* apply_chroma_compression after the post stage                      */
    float chroma_keep;         /*   float32(1 - strength), the factor animal_utils.py:181 multiplies by */
    int32_t variant;           /* 0 = auto; A/B only: 1 = reference kernel, 2 = 2-D tiled, 3 = marching strip */
    const float* streak_rows_host; /* AVX_POST_STREAK: H x streak_stride floats, per image row:
                                  [0] k1, [1] k2 (odd tap counts of the sigmaX / sigmaY kernels of that row),
                                  [2..15) k1 float32 taps, [15..48) k2 float32 taps                         */
    int32_t streak_stride;     /* >= 48                                                                  */
    int32_t in_f32;            /* 1: in_hwc is a float32 HWC frame already normalised to [0,1] (e.g. the output of
                                  avx_binocular_warp_u8); decoded with the sRGB EOTF in float32 (device powf)   */
} avx_dichromat_desc;

#define AVX_MAX_KSIZE 33

int avx_dichromat_u8(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_hwc, int n_frames, int H, int W,
                     const avx_dichromat_desc* desc, void* stream);

/* Which kernel and launch geometry the LAST avx_dichromat_u8 call on this ctx used (host state only, no device work; filled
 * by every call that got as far as choosing a kernel).  Read-only: for tests and tools that pin a geometry (AVX_MARCH_NG,
 * AVX_MARCH_CHUNKS, AVX_MARCH_SWCAP) and need to see that the pin took effect.  Fields that do not apply to a family are 0. */
enum { AVX_LAUNCH_NONE = 0, AVX_LAUNCH_REFERENCE = 1, AVX_LAUNCH_TILED = 2, AVX_LAUNCH_MARCH = 3, AVX_LAUNCH_STREAK = 4 };

typedef struct avx_dichromat_launch_info {
    uint32_t struct_size;  /* sizeof(avx_dichromat_launch_info), set by the caller                                  */
    int32_t family;        /* AVX_LAUNCH_*                                                                           */
    int32_t R;             /* blur radius (ksize / 2); 0 for the row-gain, streak and no-post stages                 */
    int32_t f64;           /* 1: float64 arithmetic (AVX_COLOR_CAT_MERGE), 0: float32                                */
    int32_t NG;            /* marching: column groups per workgroup (64: 192 compute threads, 128: 384)              */
    int32_t spec;          /* marching: 1 = wave-specialised form (one producer wave more)                           */
    int32_t sw, nstrips;   /* marching: nominal strip width in pixels, strips per frame row                          */
    int32_t ch, nchunks;   /* marching: rows per chunk, row chunks per (frame, strip)                                */
    int32_t xcd_remap;     /* marching: 1 = workgroups b and b + 8 are neighbours                                    */
    int32_t narrow;        /* marching: 1 = the narrowed strips (tuner's choice or AVX_MARCH_SWCAP below the full width) */
    int32_t tuned_now;     /* marching: 1 = this call ran a timing pass (workgroup width and / or row chunks)        */
    int32_t grid;          /* workgroups launched (every family)                                                     */
    int32_t per_cu;        /* streak, tiled, marching: resident workgroups per CU the grid / fallback was sized with */
} avx_dichromat_launch_info;

int avx_dichromat_last_launch(avx_ctx* ctx, avx_dichromat_launch_info* out);

/* The dichromats at night (csrc/night.hip): apply_rod_vision (animals/animal_utils.py:261-305) between the decode and
 * the colour stage -- the commented night branch of animals/cat.py:50-60 -- and, with bloom_strength > 0, apply_tapetum_bloom
 * (animal_utils.py:183-204, sigma 3.0) between the chroma compression and the encode.  Everything else is avx_dichromat_u8's
 * pipeline with the same avx_dichromat_desc (in_f32 = 1: float32 HWC sRGB frames in [0, 1], Cat after avx_binocular_warp_u8; variant
 * is ignored).  Float32 throughout, codes within +-1 of the reference's arithmetic (device powf; Cat's float64 tail is rounded to
 * float32 planes); the encode is the float32 threshold table.
 * Per group of frames: k_night_front -> [avx_planes_gaussian_blur_batch | avx_streak_planes_f32 per frame] -> k_night_back, all on
 * `stream`, nothing synchronises once the stream workspace's scratch holds the planes (12 B per pixel and frame, 24 B with a Gaussian
 * or streak post stage; a batch is walked in groups of at most 16 frames and at most 1 GiB of scratch, AVX_NIGHT_GROUP=n forces
 * groups of n).  Every frame's bytes are the same in any batch and any grouping.
 * AVX_ERR_INVALID (avx_last_error starts with the function's name): NULL pointers, a desc of the wrong struct_size, H or W below 13
 * (one BORDER_REFLECT_101 reflection must cover the 12-pixel bloom radius), tap counts other than 11 and 25, parameters out of range. */
typedef struct avx_night_desc {
    uint32_t struct_size;          /* sizeof(avx_night_desc)                                                      */
    double chroma_scale;           /* 0..1: x = L (1 - chroma_scale) + x chroma_scale                              */
    double luminance_boost;        /* > 0                                                                         */
    double gamma;                  /* > 0: clip(x boost, 0, 1) ** gamma                                           */
    int32_t rod_ksize;             /* 11: cv2.GaussianBlur((0, 0), 1.2) of the scotopic luminance                  */
    const double* rod_taps_host;   /* rod_ksize normalised taps in double (getGaussianKernel), like taps_host      */
    double bloom_strength;         /* 0: no bloom; else 0 < S <= 1                                                */
    int32_t bloom_ksize;           /* 25: cv2.GaussianBlur((0, 0), 3.0) of the mask and the frame                  */
    const double* bloom_taps_host; /* bloom_ksize taps in double; read only when bloom_strength > 0               */
} avx_night_desc;

int avx_dichromat_night_u8(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_hwc, int n_frames, int H, int W,
                           const avx_dichromat_desc* desc, const avx_night_desc* night, void* stream);

/* Day or night, per frame (csrc/daynight.hip): the one day/night rule the reference implements, RatUV._choose_mode
 * (animals/rat_uv.py:99-104) -- a frame is night when the median Rec.709 luma of its sRGB values is below a threshold (0.12 there).
 * For a uint8 frame Y = (t0[R] + t1[G]) + t2[B] in float32 with t_c[v] = float32(w_c * float32(v / 255)), w = (0.2126, 0.7152,
 * 0.0722): the values NumPy forms for `0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]` on x = u8.astype(float32) / 255.
 * The three tables are avx_get_table(3): 768 floats.
 * One pass gives the decision exactly.  With n = H * W and T = threshold the record of a frame holds
 *   below            #{Y < T}, compared as double
 *   max_below        the largest Y counted in `below`      (0 when below == 0)
 *   min_at_or_above  the smallest Y not counted            (+inf when below == n)
 * and the frame is night iff  2 * below > n,  or  2 * below == n and float32(max_below + min_at_or_above) / 2 < T: the median of an
 * even count is the float32 mean of its two middle values, which are then exactly these two.  avx_luma_mode_finish is that rule on
 * the host (no device call; ctx may be NULL).
 * avx_luma_mode_u8: asynchronous on `stream`; one launch that initialises the n_frames records and one launch of grid (chunks,
 * frames) that reduces per wave, then per workgroup, and applies three integer atomics per workgroup (add, unsigned max and min
 * on the bit patterns: Y >= 0), so a frame's record is the same bytes in any batch and any grid.  1 <= n_frames <= 16, H, W >= 1,
 * H * W < 2^31, 0 <= threshold <= 1; rec_dev is device memory, 16-byte aligned. */
typedef struct avx_luma_mode_rec {
    uint32_t below;
    float max_below;
    float min_at_or_above;
    uint32_t pad_;
} avx_luma_mode_rec;

int avx_luma_mode_u8(avx_ctx* ctx, const uint8_t* in_hwc, int n_frames, int H, int W, double threshold, avx_luma_mode_rec* rec_dev,
                     void* stream);
int avx_luma_mode_finish(avx_ctx* ctx, const avx_luma_mode_rec* rec_host, int n_frames, int H, int W, double threshold, uint8_t* modes_host);

/* The dichromats, switched per frame: avx_luma_mode_u8 on the n_frames uint8 frames, the 16-byte records into pinned memory of the
 * stream's workspace, hipStreamSynchronize(stream) -- that stream only; a stated cost --, the decision on the host, then
 * avx_dichromat_u8 on every maximal run of day frames and avx_dichromat_night_u8 on every maximal run of night frames, with the
 * pointers at the run's first frame.  A frame's bytes are what that entry writes for the frame alone.  modes_host (may be NULL)
 * receives 1 for night, 0 for day.  1 <= n_frames <= 16.  AVX_ERR_INVALID, by name: desc->in_f32 (the decision is defined on
 * uint8 frames), H or W below 13 (as the night entry, also when every frame is day), and whatever the two entries refuse. */
int avx_dichromat_auto_u8(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_hwc, int n_frames, int H, int W,
                          const avx_dichromat_desc* desc, const avx_night_desc* night, double threshold, uint8_t* modes_host, void* stream);

/* ---- UV / spectral path: uv_helpers.py, uv_mappers.py, ml/classic_rgb_to_hsi, animals/honeybee.py ----
 *
 * Planes are float32, K x (H*W), struct-of-arrays.  Float contract: within 1e-4 relative of the reference
 * (device atan2f/powf); order statistics are exact; uint8 encode uses the reference's threshold table. */

/* np.percentile(data, q) with linear interpolation (uv_mappers.py:32,61-62,73,104,142): exact order
 * statistics by radix select on device, NumPy's _lerp formula; blocks until the value is on the host. */
int avx_percentile(avx_ctx* ctx, const float* data, size_t n, double q, double* out_host, void* stream);

/* integrate_band / cone catches (uv_helpers.py:142-146, honeybee.py:125-135): out_k = sum_b hsi_b * w[k][b].
 * layout 0 = HxWxB (NHWC), 1 = BxHxW (NCHW, what a torch model emits); dtype 0 = float32, 1 = float16.
 * weights_host: K x B with the illuminant already folded in.  stats_host (optional): K x {min,max,mean,1}. */
int avx_spectral_integrate(avx_ctx* ctx, const void* hsi, int layout, int dtype, int H, int W, int B,
                           const float* weights_host, int K, float* out_planes, float* stats_host, void* stream);

/* {min, max, mean, denominator} per plane (safe_norm uv_helpers.py:47-53, von_kries_* :195-206).
 * adapt: 0 none (den 1), 1 white_patch max(max,eps), 2 gray_world max(mean,eps), 3 safe_norm (max-min).
 * The result stays on the device for the next avx_planes_gaussian_blur; stats_host (optional) copies it. */
int avx_plane_stats(avx_ctx* ctx, const float* planes, int K, size_t n, int adapt, float eps, float* stats_host, void* stream);

/* uv_helpers.gaussian_blur (uv_helpers.py:67-73, cv2 semantics) on K planes, optionally rescaling each plane by
 * the statistics of the last avx_plane_stats / avx_spectral_integrate first: scale_mode 0 none, 1 x/den,
 * 3 safe_norm.  ksize == 1: rescale only.  taps_host: ksize normalised taps in double. */
int avx_planes_gaussian_blur(avx_ctx* ctx, const float* in, float* out, int K, int H, int W, int ksize,
                             const double* taps_host, int scale_mode, void* stream);
/* The same for n_frames (<= AVX_EW_MAX_FRAMES) frames of K planes in one launch: frame f at in + f * in_frame_stride /
 * out + f * out_frame_stride (in floats, >= K*H*W).  scale_mode must be 0 when n_frames > 1 (the statistics are one frame's). */
int avx_planes_gaussian_blur_batch(avx_ctx* ctx, const float* in, size_t in_frame_stride, float* out, size_t out_frame_stride,
                                   int n_frames, int K, int H, int W, int ksize, const double* taps_host, int scale_mode,
                                   void* stream);

/* apply_anisotropic_acuity_blur_with_streak (animals/animal_utils.py:147-172, as coded: quirk Q3) on three float32
 * planes of linear light (3 x H x W in, 3 x H x W out): the float-frame form of the streak species; uint8 frames take
 * the fused avx_dichromat_u8.  rows_host: H x stride floats per image row [k1, k2, 13 taps(sigma_x), 33 taps(sigma_y)]. */
int avx_streak_planes_f32(avx_ctx* ctx, const float* src_planes, float* dst_planes, int H, int W, const float* rows_host,
                          int stride, void* stream);

/* classic_rgb_to_hsi analytic branch (ml/classic_rgb_to_hsi/classic_rgb_to_hsi.py:47-82): HxWx3 frame (uint8, or
 * float32 that is linearised as coded) -> HxWxB float32 cube.  gains_host: B x 3 lobe gains in input-channel
 * order (quirk Q5), denom: mean lobe sum + 1e-8. */
int avx_rgb_to_hsi_lobes(avx_ctx* ctx, const void* in_hwc, int in_is_u8, int H, int W, int B, const float* gains_host,
                         float denom, float* out_hwb, void* stream);

/* HoneyBee.visualize steps 1-7 (animals/honeybee.py:99-175) for N uint8 frames, all passes on the device:
 * catches -> von Kries -> Gaussian blur -> percentiles -> map_* -> clip -> OETF -> uint8. */
enum { AVX_MAP_FALSECOLOR = 0, AVX_MAP_CUSTOM_MATRIX = 1, AVX_MAP_OPPONENT = 2, AVX_MAP_UV_PURPLE_YELLOW = 3, AVX_MAP_FALSECOLOR_UV_MIXED = 4 };
typedef struct avx_honeybee_desc {
    uint32_t struct_size;
    int32_t source;            /* 0: uint8 RGB frames + rgb_matrix (analytic lobes x illuminant x cone curves folded
                                  to 3x3, the route honeybee.py actually takes); 1: an HSI cube + weights_host;
                                  2: the catches themselves + their statistics (one frame)                        */
    float rgb_matrix[9];       /* source 0: [U,B,G]_k = sum_j rgb_matrix[k][j] * linear_channel_j                  */
    const void* hsi;           /* source 1: device cube(s), N of them back to back                                */
    int32_t hsi_layout, hsi_dtype, bands;
    const float* weights_host; /* source 1: 3 x bands (illuminant folded in)                                      */
    int32_t adaptation;        /* 0 none, 1 white_patch, 2 gray_world (honeybee.py:137-141)                       */
    float eps;
    int32_t blur_ksize;        /* 0: no blur; else odd taps of uv_helpers.gaussian_blur                            */
    const double* blur_taps_host;
    int32_t mapping;           /* AVX_MAP_*                                                                       */
    float custom_matrix[9];
    float mixed_alpha;         /* falsecolor_uv_mixed alpha (honeybee.py:162 passes 0.45)                          */
    int32_t out_float;         /* 1: out_hwc is a float32 HxWx3 buffer receiving linear_to_srgb(clip(rgb_lin)) (the
                                  reference's output for float frames, honeybee.py:172-173) instead of uint8 codes */
    const float* catches;      /* source 2: the three catch planes (device, 3 x H*W float32) already formed, e.g. by
                                  avx_mst_conv3x3_lds_spectral (the spectral integration as conv_out's epilogue) ...  */
    const void* catch_partials; /* ... with n_catch_partials x 3 records {float min, max; double sum} of them (device) */
    int32_t n_catch_partials;
} avx_honeybee_desc;

/* debug_planes (optional, device, N x 3 x H*W floats): receives U,B,G after adaptation + blur. */
int avx_honeybee_u8(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_hwc, int n_frames, int H, int W,
                    const avx_honeybee_desc* desc, float* debug_planes, void* stream);

/* The three catch planes formed at reduced size (planes_small: 3 x h*w float32, device) enlarged to the frame (planes_out: 3 x H*W),
 * h <= H and w <= W, with the statistics of the enlarged planes, in one launch (HoneyBee(hsi_model=, hsi_downsample=True)).
 * Plane k of planes_out is, bit for bit, avx_resize_hwc(plane k, dtype 0, h, w, C = 1, out, H, W, interp 1): cv2's float32 INTER_LINEAR
 * with the same tables (h == H and w == W: that resize's values, the plane itself).  partials_out (device, 16-byte aligned, room for
 * 8 x CUs x 3 records of 16 bytes) receives *n_partials x 3 records {float min, max; double sum}, one triple per workgroup, no atomics:
 * feed planes_out and them to avx_honeybee_u8 (source 2).  AVX_ERR_INVALID (avx_last_error starts with the function's name) for NULL
 * pointers, non-positive sizes, h > H or w > W, overlapping buffers and a misaligned partials_out. */
int avx_catch_planes_up(avx_ctx* ctx, const float* planes_small, int h, int w, float* planes_out, int H, int W, void* partials_out, int* n_partials,
                        void* stream);

/* ---- geometric resampling: cv2.resize / cv2.remap / cv2.Sobel call sites ----------------
 * OpenCV semantics restated from its published algorithm (OpenCV is not available to pin against). */

/* cv2.resize(src, (Wd, Hd), interpolation) on an HWC image (uv_helpers.py:57-64,94,172,182;
 * cat_widevision_utils.py:26).  dtype 0 = float32 (interp 1 LINEAR, 2 CUBIC a=-0.75, 3 AREA), 2 = uint8 (LINEAR,
 * 11-bit fixed point). */
int avx_resize_hwc(avx_ctx* ctx, const void* src, int dtype, int H, int W, int C, void* dst, int Hd, int Wd, int interp, void* stream);

/* animal_fov_binocular_warp (cat_widevision_utils.py:46-99) on a uint8 frame: get_normalized_image, two
 * cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) with per-column x maps / per-row y map, cos^2 blend weights, clip:
 * -> float32 HWC in [0,1].  Host tables: xL, xR, wL, wR (Wo floats each), ymap (Ho floats). */
int avx_binocular_warp_u8(avx_ctx* ctx, const uint8_t* in_hwc, int H, int W, const float* xL_host, const float* xR_host, const float* ymap_host,
                          const float* wL_host, const float* wR_host, int Ho, int Wo, float* out_hwc_f32, void* stream);

/* Cat's wide view (animals/cat.py:82-109) of n_frames contiguous uint8 HWC frames in one launch (csrc/cat_wide.hip); the
 * output has the input's size.  Defined as the chain, frame by frame,
 *     avx_binocular_warp_u8(frame, H, W, tables, Ho = H, Wo = W) -> float32 frame -> avx_dichromat_u8(desc with in_f32 = 1)
 * and byte for byte equal to it on the same device.  desc: AVX_COLOR_CAT_MERGE, AVX_POST_GAUSS (odd ksize <= AVX_MAX_KSIZE) or
 * AVX_POST_NONE, no chroma compression; in_f32 and variant are ignored.  d_xL, d_xR, d_wL, d_wR (W floats each) and d_ymap (H floats)
 * are DEVICE pointers the caller owns and keeps alive until the work has run (geometry.binocular_warp_tables' vectors).  Asynchronous on
 * `stream`: a memset, one pass that finds each frame's "any byte > 1" flag and the fused launch -- no stream synchronisation, no
 * host-to-device copy and, once the stream workspace holds n_frames flags, no allocation.  AVX_ERR_INVALID (avx_last_error starts
 * with the function's name) for NULL pointers, n_frames < 0, H or W <= 0 and a desc of the wrong struct_size, colour mode, post mode
 * or ksize; n_frames == 0 is AVX_OK without a launch. */
int avx_cat_wide_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, const avx_dichromat_desc* desc,
                    const float* d_xL, const float* d_xR, const float* d_ymap, const float* d_wL, const float* d_wR, void* stream);

/* The wide view of any dichromat (csrc/dichromat_wide.hip): avx_cat_wide_u8's definition with any dichromat desc --
 * AVX_COLOR_MATRIX or AVX_COLOR_CAT_MERGE; AVX_POST_NONE, _GAUSS (odd ksize <= AVX_MAX_KSIZE), _ROWGAIN or _STREAK; chroma
 * compression on or off; in_f32 and variant are ignored.  For NONE, GAUSS and ROWGAIN every frame is byte for byte the chain
 *     avx_binocular_warp_u8(frame, H, W, tables, Ho = H, Wo = W) -> float32 frame -> avx_dichromat_u8(desc with in_f32 = 1)
 * on the same device.  AVX_POST_STREAK (AVX_COLOR_MATRIX only) has no such chain: warp, blend, float32 sRGB decode and the matrix
 * -> three float32 planes, avx_streak_planes_f32 per frame, chroma compression, the float32 threshold encode; codes within +-1 of
 * the reference's arithmetic (device powf).  Two routes compute the same bytes: one fused tile kernel, or planes in the stream
 * workspace's scratch (12 B per pixel and frame, 24 B with a Gaussian or streak post stage; a batch is walked in groups of at most
 * 16 frames and 1 GiB).  The entry picks by post stage and radius; AVX_WIDE_ROUTE=fused|planes, AVX_WIDE_TILE=WxH (the fused
 * kernel's tile) and AVX_WIDE_GROUP=n (frames per group) are tuning and test switches.  STREAK always takes the planes route,
 * AVX_COLOR_CAT_MERGE (float64) always the fused one.
 * Tables and call discipline as avx_cat_wide_u8: device pointers the caller owns; asynchronous on `stream`, no stream
 * synchronisation and no copy of the warp tables (the row gains and the streak row tables are host tables of the desc and are
 * uploaded when they differ from the last call's, like avx_dichromat_u8's).  AVX_ERR_INVALID (avx_last_error starts with the
 * function's name) for NULL or aliased frame pointers, NULL tables, n_frames < 0, H or W <= 0 and a desc of the wrong struct_size,
 * colour mode, post mode, ksize or missing host tables; n_frames == 0 is AVX_OK without a launch. */
int avx_dichromat_wide_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, const avx_dichromat_desc* desc,
                          const float* d_xL, const float* d_xR, const float* d_ymap, const float* d_wL, const float* d_wR, void* stream);

/* center_zoom (cat_widevision_utils.py:11-29) of n_frames contiguous uint8 HWC frames in one launch: each output frame is
 * cv2.resize(frame[y0:y0+ch, x0:x0+cw], (W, H), INTER_LINEAR), byte for byte avx_resize_hwc(dtype 2, interp 1) of the contiguous crop,
 * with that call's tables (the stream workspace's cache: built and uploaded the first time a geometry is seen); the crop is read in
 * place through the frame's row stride.  AVX_ERR_INVALID for NULL or aliased pointers, n_frames < 0, H or W <= 0, cw or ch < 1 and a
 * crop that leaves the frame, before any launch; n_frames == 0 is AVX_OK without a launch. */
int avx_center_zoom_u8(avx_ctx* ctx, const uint8_t* in_hwc_u8, uint8_t* out_hwc_u8, int n_frames, int H, int W, int x0, int y0, int cw, int ch,
                       void* stream);

/* VideoRenderer.make_split_frame (renderers/video.py:198-245) for two frames of the same size, without the
 * Hershey-font labels: left half `original`, right half `modified`, optional 1-px white seam at W//2.
 * out_hwc may alias modified_hwc (each byte is read before it is written by the same thread). */
int avx_split_compose_u8(avx_ctx* ctx, const uint8_t* original_hwc, const uint8_t* modified_hwc, uint8_t* out_hwc,
                         int H, int W, int draw_seam, void* stream);

/* VideoRenderer._draw_label (renderers/video.py:160-196) on a device-resident uint8 frame, in place: the 60 % black box
 * (inside box_xyxy, inclusive corners: out = saturate_cast<uchar>(0.4 * in)), then the text as stroke segments -- black at
 * outline_thickness, white at text_thickness (cv2.putText x 2, :194-195).  segments_host: n x 6 floats per segment
 * {ax, ay, bx - ax, by - ay, 1 / |b - a|^2 (0 for a point), 0} in pixel coordinates, built by the host from the Hershey
 * simplex stroke tables with the reference's geometry (renderers/labels.py).  Anti-aliasing is analytic distance coverage, not
 * OpenCV's LINE_AA scan converter (label pixels: parity unpinned; geometry pinned).  slot (0 | 1) names which of two cached
 * device copies of the segment table the call may reuse (a frame has two labels). */
int avx_draw_label_u8(avx_ctx* ctx, uint8_t* img_hwc, int H, int W, const int box_xyxy[4], const float* segments_host, int n_segments,
                      float outline_thickness, float text_thickness, int slot, void* stream);

/* One tile of a labelled contact sheet (avx_gallery_compose_u8). */
typedef struct avx_gallery_tile {
    const void* src;           /* device, C-contiguous H x W x 3                                               */
    int32_t dtype;             /* 0 float32 (clipped to [0, 1], then * 255 + 0.5, truncated), 2 uint8           */
    int32_t H, W;              /* source size                                                                   */
    int32_t h, w;              /* resized size: (H, W) = no resize; else INTER_AREA (INTER_LINEAR when enlarging) */
    int32_t seg_offset, seg_count;  /* this tile's label: rows of the concatenated segment table               */
} avx_gallery_tile;

/* gallery_grid.build_labeled_grid (gallery_grid.py:8-106) after the host has laid it out, in ONE launch that writes every
 * byte of the Hc x Wc x 3 uint8 canvas once.  Tile i sits in cell (i / cols, i % cols) of (max h + strip_h + pad) x
 * (max w + pad) pixels, at (pad + row * cell_h, pad + col * cell_w); it is its source resized to h x w with avx_resize_hwc's
 * arithmetic (cv2.resize INTER_AREA), a black strip of strip_h rows below it, and its label drawn on that (h + strip_h) x w
 * image exactly as avx_draw_label_u8 draws it with the box (0, h, w - 1, h + strip_h - 1), outline 3 and text 1
 * (_label_strip: the text is clipped to the tile).  The segments ({ax, ay, dx, dy, 1 / len^2, 0} rows, avx_draw_label_u8's
 * format) are in the coordinates of that tile-plus-strip image, the label origin applied.  Every other byte is bg.  The
 * canvas must not overlap a source. */
int avx_gallery_compose_u8(avx_ctx* ctx, const avx_gallery_tile* tiles_host, int n_tiles, const float* segments_host, int n_segments,
                           int strip_h, int pad, int cols, const int bg_rgb[3], uint8_t* canvas_hwc, int Hc, int Wc, void* stream);

/* The species wall: avx_gallery_compose_u8's sheet for a batch of video frames whose tiles are all uint8 H x W x 3
 * sources of one size, resized to one h x w.  A layout holds everything that does not change from frame to frame -- the resize
 * mode (avx_gallery_compose_u8's choice: copy, integer-ratio INTER_AREA, general INTER_AREA, INTER_LINEAR when enlarging), the
 * axis tables, the label segments of the n_tiles tiles (seg_offset / seg_count: rows of segments_host per tile; both may be NULL
 * with n_segments == 0) and the grid -- on the device.  avx_wall_layout_create is the only call here that allocates, uploads
 * and synchronises.  The canvas is the gallery's (rows * cell_h + pad) x (cols * cell_w + pad) with each dimension rounded up to
 * even; the added row or column is bg (4:2:0 sinks get even sizes). */
typedef struct avx_wall_layout avx_wall_layout;
int avx_wall_max_tiles(void);                       /* tiles one layout takes (source pointers are kernel arguments): 64 */
int avx_wall_layout_create(avx_ctx* ctx, int H, int W, int h, int w, int n_tiles, const int* seg_offset, const int* seg_count,
                           const float* segments_host, int n_segments, int strip_h, int pad, int cols, const int bg_rgb[3],
                           avx_wall_layout** out_layout);
int avx_wall_layout_destroy(avx_ctx* ctx, avx_wall_layout* layout);
int avx_wall_canvas_size(const avx_wall_layout* layout, int* Hc, int* Wc);
/* What the layout chose (each pointer may be NULL): mode 0 copy / 1 integer-ratio area / 2 area / 3 linear; staged: 1 when a
 * workgroup's band of source rows goes through LDS, 0 when it does not fit and the samples read the source; the pixels of one
 * workgroup's piece of a canvas row; the dynamic LDS of a workgroup in bytes. */
int avx_wall_layout_info(const avx_wall_layout* layout, int* mode, int* staged, int* piece_px, size_t* lds_bytes);
/* n_frames (<= AVX_EW_MAX_FRAMES) canvases in ONE launch (the frame is a grid dimension): frame f of tile i is read at
 * src[i] + f * src_frame_stride, its canvas written at canvas + f * canvas_frame_stride (strides in bytes, >= a frame).  src is a
 * host array of the layout's n_tiles device pointers; they travel as kernel arguments, so the call does no copy, no allocation
 * and no synchronisation.  Every canvas is byte for byte what avx_gallery_compose_u8 writes for the same tiles, labels, strip_h,
 * pad, cols and bg on the gallery's extent, and bg outside it.  n_frames == 0: AVX_OK, nothing launched.  AVX_ERR_INVALID before
 * any launch: NULL pointers, a source overlapping the canvas, strides below a frame, n_frames above the cap, a layout of another
 * context. */
int avx_wall_compose_u8(avx_ctx* ctx, const avx_wall_layout* layout, const uint8_t* const* src, size_t src_frame_stride, int n_frames,
                        uint8_t* canvas, size_t canvas_frame_stride, void* stream);

/* YUV 4:2:0 <-> RGB (Y4M video I/O).  `yuv` is the Y4M payload of n_frames frames back to back: a Y plane of H x W, then U,
 * then V, each ceil(H/2) x ceil(W/2), no padding; `rgb_hwc` is n_frames x H x W x 3.  int32 fixed point with 16 fractional
 * bits: decode clamp((sum c_i x_i + 2^15) >> 16, 0, 255) with x = (Y - yo, U - 128, V - 128) and chroma replicated
 * over its 2x2 block; encode Y per pixel, U / V from the 2x2 block sums (an odd last column / row replicated) with
 * 128 + ((sum c_i S_i + 2^17) >> 18).  matrix: AVX_YUV_BT601 (default of OpenCV and swscale) or AVX_YUV_BT709; full_range 0 =
 * limited (Y 16..235, chroma scale 224/255), 1 = full.  Chroma siting is ignored.  The buffers must not overlap. */
enum { AVX_YUV_BT601 = 0, AVX_YUV_BT709 = 1 };
int avx_i420_to_rgb_u8(avx_ctx* ctx, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int matrix, int full_range, void* stream);
int avx_rgb_to_i420_u8(avx_ctx* ctx, const uint8_t* rgb_hwc, uint8_t* yuv, int n_frames, int H, int W, int matrix, int full_range, void* stream);
/* The coefficient tables those two kernels run with (host only, no ctx, no device): dec_out = {cy, crv, cgu, cgv, cbu, yo}
 * (R = cy y + crv v, G = cy y + cgu u + cgv v, B = cy y + cbu u), enc_out = {Y row r g b, U row r g b, V row r g b, yo}. */
int avx_yuv_coefficients(int matrix, int full_range, int dec_out[6], int enc_out[10]);

/* Raw video pixel formats (csrc/yuv_raw.hip), named as ffmpeg's -pix_fmt names them.  One frame of H x W, with
 * cw = ceil(W/2) and ch = ceil(H/2), no padding, frames back to back:
 *   YUV420P  Y, U (ch x cw), V (ch x cw), 8-bit: the I420 payload above      NV12    Y, then ch rows of cw (U, V) byte pairs
 *   YUV422P  Y, U (H x cw), V (H x cw)        YUV444P  Y, U, V (H x W each)  GRAY    Y only (decodes with neutral chroma)
 *   YUV4xxP10LE  as the 8-bit planar forms, every sample a little-endian uint16 holding 0..1023
 *   P010LE   as NV12, every sample a little-endian uint16 with the 10-bit value in its high bits (value << 6); the low 6 bits
 *            are ignored on read and written as zero
 * A payload is always addressed as bytes.  The arithmetic is that of the I420 pair at sample depth d = 8 or 10: yo = 16 s,
 * ys = 219 s / 255, cs = 224 s / 255 with s = 2^(d-8) (limited) or yo = 0, ys = cs = (2^d - 1) / 255 (full), the chroma centre
 * 2^(d-1), outputs clamped to 0 .. 2^d - 1, chroma from the sum over its block of n = 1, 2 or 4 pixels with
 * c + ((sum + 2^(15 + log2 n)) >> (16 + log2 n)).  At d = 8 the tables are those of avx_yuv_coefficients, so YUV420P equals the
 * I420 pair byte for byte.  The buffers must not overlap; payloads of 16-bit samples must be 2-byte aligned. */
enum avx_pix_fmt {
    AVX_PIX_YUV420P = 0, AVX_PIX_NV12 = 1, AVX_PIX_YUV422P = 2, AVX_PIX_YUV444P = 3, AVX_PIX_GRAY = 4,
    AVX_PIX_YUV420P10LE = 5, AVX_PIX_YUV422P10LE = 6, AVX_PIX_YUV444P10LE = 7, AVX_PIX_P010LE = 8, AVX_PIX_FMT_COUNT = 9
};
/* Bytes of one frame (host only); 0 for a bad format or size. */
size_t avx_yuv_frame_size(int fmt, int H, int W);
int avx_yuv_to_rgb_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int matrix, int full_range, void* stream);
int avx_rgb_to_yuv_u8(avx_ctx* ctx, int fmt, const uint8_t* rgb_hwc, uint8_t* yuv, int n_frames, int H, int W, int matrix, int full_range, void* stream);
/* avx_yuv_coefficients at sample depth 8 or 10 (host only). */
int avx_yuv_coefficients_d(int matrix, int full_range, int depth, int dec_out[6], int enc_out[10]);

/* HDR video in (csrc/yuv_hdr.hip): one of the four 10-bit formats above, BT.2020 non-constant-luminance Y'CbCr with
 * a PQ (SMPTE ST 2084) or HLG (BT.2100, OOTF at 1000 nits) transfer -> tone-mapped SDR sRGB, interleaved RGB uint8 as
 * avx_yuv_to_rgb_u8 writes it.  Per pixel: R'G'B' clamped to [0, 1] -> display light / sdr_white -> all three channels scaled by
 * t(m) / m, m their maximum (CLIP: t = min(m, 1); MOBIUS: the identity below 0.75, a Moebius curve above it that reaches 1 at
 * peak_nits / sdr_white) -> BT.2020 to BT.709 primaries -> clamp -> sRGB encode.  The matrix is always BT.2020; peak_nits >
 * sdr_white > 0, both finite.  An 8-bit format or GRAY, a bad transfer or tonemap, NULL or overlapping buffers, an odd payload
 * address or a bad size return AVX_ERR_INVALID. */
enum avx_transfer { AVX_TRANSFER_PQ = 1, AVX_TRANSFER_HLG = 2 };
enum avx_tonemap { AVX_TONEMAP_CLIP = 0, AVX_TONEMAP_MOBIUS = 1 };
int avx_yuv_hdr_to_rgb_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int full_range, int transfer,
                          int tonemap, double peak_nits, double sdr_white, void* stream);

/* Scaled decode (csrc/yuv_scale.hip): n_frames payloads of avx_yuv_frame_size(fmt, H, W) bytes -> n_frames frames of
 * Hd x Wd interleaved RGB uint8 (n_frames * Hd * Wd * 3 bytes), 1 <= Hd <= H, 1 <= Wd <= W, in one launch.  Per frame the result
 * is, byte for byte,
 *     avx_resize_hwc(avx_yuv_to_rgb_u8(fmt, frame, H, W, matrix, full_range), dtype = 2 (uint8), C = 3, Hd, Wd, interp = 3 (INTER_AREA))
 * without the full-size RGB frame ever being written: the decode of avx_yuv_to_rgb_u8 (chroma replicated over its block), then
 * cv2's INTER_AREA -- when W / Wd and H / Hd are both integers, the integer sum of each isx x isy block per channel, rounded as
 * (sum + 2) >> 2 for 2 x 2 and as rint(sum * (1.f / (isx * isy))) (half to even) otherwise; for any other ratio the float32
 * weighted sums of avx_resize_hwc's general path, with its tables, in its order.  Hd == H and Wd == W gives avx_yuv_to_rgb_u8's
 * frame.  AVX_ERR_INVALID (avx_last_error starts with the function's name) for a bad format, matrix, range or size, Hd > H or
 * Wd > W (enlarging is not supported), an integer-ratio block of more than 65536 samples, NULL or overlapping buffers, and an odd
 * payload address with a 16-bit format. */
int avx_yuv_to_rgb_scaled_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int Hd, int Wd, int matrix,
                             int full_range, void* stream);

/* Scaled HDR decode (csrc/yuv_hdr_scale.hip): n_frames 10-bit payloads of avx_yuv_frame_size(fmt, H, W) bytes ->
 * n_frames frames of Hd x Wd interleaved RGB uint8 (n_frames * Hd * Wd * 3 bytes), 1 <= Hd <= H, 1 <= Wd <= W, in one launch.  Per
 * frame the result is, byte for byte,
 *     avx_resize_hwc(avx_yuv_hdr_to_rgb_u8(fmt, frame, H, W, full_range, transfer, tonemap, peak_nits, sdr_white),
 *                    dtype = 2 (uint8), C = 3, Hd, Wd, interp = 3 (INTER_AREA))
 * without the full-size RGB frame ever being written: every source pixel is decoded to its three uint8 codes exactly as
 * avx_yuv_hdr_to_rgb_u8 decodes it, and cv2's INTER_AREA reduces those codes as avx_yuv_to_rgb_scaled_u8 describes (integer ratios:
 * the integer block sum, (sum + 2) >> 2 for 2 x 2 and rint(sum * (1.f / (isx * isy))) otherwise; any other ratio: the float32
 * weighted sums of avx_resize_hwc's general path).  Hd == H and Wd == W gives avx_yuv_hdr_to_rgb_u8's frame.  AVX_ERR_INVALID
 * (avx_last_error starts with this function's name) for everything either of the two refuses: an 8-bit format or GRAY, a bad
 * transfer, tonemap or range, peak_nits <= sdr_white or a non-finite or non-positive value, a bad size, Hd > H or Wd > W, an
 * integer-ratio block of more than 65536 samples, NULL or overlapping buffers, and an odd payload address. */
int avx_yuv_hdr_to_rgb_scaled_u8(avx_ctx* ctx, int fmt, const uint8_t* yuv, uint8_t* rgb_hwc, int n_frames, int H, int W, int Hd, int Wd,
                                 int full_range, int transfer, int tonemap, double peak_nits, double sdr_white, void* stream);

/* Frame comparison (csrc/metrics.hip): what two batches of uint8 RGB frames differ by, per frame and channel. */
typedef struct avx_frame_metrics {
    uint32_t abs_hist[3][256]; /* [c][k]: samples of channel c with |a - b| == k; each row sums to H*W */
    double   ssim[3];          /* mean SSIM of channel c over the (H-10) x (W-10) window positions;    */
                               /* NaN when with_ssim == 0 or H < 11 or W < 11                          */
} avx_frame_metrics;

/* a_hwc, b_hwc: n_frames contiguous H x W x 3 uint8 frames on the device; out_dev: n_frames records on the device (8-byte aligned).
 * Asynchronous on `stream`.  1 <= n_frames <= 16, H*W < 2^32.  The histogram is exact and covers every sample: SSE, PSNR, the
 * largest difference and the share of samples beyond +-k codes follow from it without rounding.  SSIM is Wang et al. 2004 as
 * skimage computes it with gaussian_weights=True, use_sample_covariance=False: per channel an 11 x 11 separable Gaussian window,
 * sigma 1.5, taps normalised to sum 1 in float64; valid positions only; C1 = (0.01*255)^2, C2 = (0.03*255)^2;
 * (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2)) with s^2 = E[x^2] - mu^2; the mean over positions.
 * The moments and the quotient are float32, on samples centred by 128; every sum over positions is float64 in a fixed order
 * (no floating-point atomics): a frame's record is bit-identical whichever batch and batch position it was computed in, and from run
 * to run; identical frames give exactly 1.0.  AVX_ERR_INVALID (avx_last_error starts with this function's name) for a NULL
 * buffer, n_frames outside 1..16 and a bad size; nothing is launched then. */
int avx_frame_metrics_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W,
                         int with_ssim, avx_frame_metrics* out_dev, void* stream);

/* Comparison in YUV planes (csrc/plane_metrics.hip): what two batches of video payloads differ by, per frame and
 * plane, in their own samples: no matrix, no range, no chroma upsampling, no rounding to 8 bits. */
typedef struct avx_plane_metrics_rec {
    uint32_t abs_hist[3][1024]; /* [p][k], p = Y, U, V: samples of plane p with |a - b| == k; 8-bit formats use bins 0..255 */
    double   ssim[3];           /* mean SSIM of plane p over its (h_p - 10) x (w_p - 10) window positions; NaN when with_ssim == 0, */
                                /* the plane is absent (GRAY: U, V) or smaller than 11 in either dimension                          */
} avx_plane_metrics_rec;

/* a, b: n_frames payloads of avx_yuv_frame_size(fmt, H, W) bytes on the device, in any avx_pix_fmt layout; fmt_a and fmt_b may
 * differ where they agree in sample depth and chroma subsampling (YUV420P against NV12, YUV420P10LE against P010LE).  out_dev:
 * n_frames records on the device (8-byte aligned).  Asynchronous on `stream`.  1 <= n_frames <= 16.  Samples are read as the
 * decoders read them: bytes at 8 bits, little-endian uint16 at 10 bits, P010LE shifted right by 6 (its low six bits are ignored).
 * A planar 10-bit sample above 1023 is invalid input: its difference is clamped into bin 1023, so no count is ever written outside
 * the histogram.  Plane sizes: Y is H x W, U and V are ceil(H / 2^sy) x ceil(W / 2^sx).  The histogram is exact and covers every
 * sample of every plane (each row sums to that plane's sample count, rows of absent planes are zero).  SSIM is that of
 * avx_frame_metrics_u8 per plane at the plane's own size, with dynamic range L = 2^d - 1: C1 = (0.01 L)^2, C2 = (0.03 L)^2.  At 8
 * bits the moments and the quotient are float32 on samples centred by 128; at 10 bits they are float64 (a fixed centre does not keep
 * float32 within 1e-5 there).  Every sum over positions is float64 in a fixed order (no floating-point atomics): a frame's record
 * is bit-identical whichever batch and batch position it was computed in, and from run to run; identical planes give exactly 1.0.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for a NULL buffer, n_frames outside 1..16, a bad format or
 * size (1 .. 32768 each way; a plane stays below 2^32 samples), formats that disagree in depth or subsampling, and an odd payload
 * address with a 16-bit format; nothing is launched then. */
int avx_plane_metrics(avx_ctx* ctx, int fmt_a, const uint8_t* a, int fmt_b, const uint8_t* b, int n_frames, int H, int W,
                      int with_ssim, avx_plane_metrics_rec* out_dev, void* stream);

/* MS-SSIM, five scales (csrc/ms_ssim.hip; Wang, Simoncelli, Bovik 2003): the per-scale means of two batches of uint8
 * RGB frames, per frame and channel.  The product over the scales is formed by the caller (metrics.MsSsim). */
typedef struct avx_ms_ssim_rec {
    double cs[3][5];   /* [c][j]: mean of cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2) over the window positions of scale j */
    double ssim[3][5]; /* [c][j]: mean of l * cs, l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1); neither is clamped  */
} avx_ms_ssim_rec;     /* 240 bytes */

/* a_hwc, b_hwc: n_frames contiguous H x W x 3 uint8 frames on the device; out_dev: n_frames avx_frame_metrics, ms_out_dev: n_frames
 * avx_ms_ssim_rec, both on the device and 8-byte aligned.  Asynchronous on `stream`; nothing waits on the host and, once the
 * stream's workspace has grown to the batch, nothing is allocated.  1 <= n_frames <= 16, H >= 176 and W >= 176 (scale 4 is
 * floor(H/16) x floor(W/16) and needs one window position), H*W < 2^32.
 * Scale 0 of a channel is the channel; scale j+1 is the 2 x 2 mean of scale j at floor(h/2) x floor(w/2), a trailing odd row or
 * column dropped -- equivalently the sum of an origin-aligned 2^j x 2^j block divided by 4^j, which is how the scales are stored:
 * exact integer sums in uint16.  At every scale the window, the constants (L = 255) and the valid positions are those of
 * avx_frame_metrics_u8.  MS-SSIM of a channel = prod_{j<4} max(cs[c][j], 0)^w_j * max(ssim[c][4], 0)^w_4 with
 * w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); the frame value is the mean of the channels.
 * out_dev receives exactly the bytes avx_frame_metrics_u8(..., with_ssim = 1, ...) writes for the same input, and
 * ms_out_dev[f].ssim[c][0] is bit-identical to out_dev[f].ssim[c]: scale 0 is that kernel's tile code, instantiated to sum cs as
 * well (float32 moments on samples centred by 128).  Scales 1..4 carry up to 8 fractional bits: their moments, the window sums
 * and the quotients are float64.  Every sum over positions is float64 in a fixed order (no floating-point atomics): a frame's
 * record is bit-identical whichever batch and batch position it was computed in, and from run to run; identical frames give
 * exactly 1.0 at every scale.  AVX_ERR_INVALID (avx_last_error starts with this function's name) for a NULL buffer, n_frames
 * outside 1..16, H or W below 176 and H*W >= 2^32; nothing is launched then. */
int avx_frame_metrics_ms_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W,
                            avx_frame_metrics* out_dev, avx_ms_ssim_rec* ms_out_dev, void* stream);

/* Difference maps (csrc/diff_map.hip): where two batches of uint8 RGB frames differ, as a picture per frame, and per
 * frame the largest difference, its first pixel and the pixels beyond a threshold. */
enum avx_diff_mode { AVX_DIFF_ABS = 0, AVX_DIFF_HEAT = 1, AVX_DIFF_SSIM = 2 };
enum avx_diff_layout { AVX_DIFF_MAP = 0, AVX_DIFF_SIDE = 1 };
typedef struct { uint32_t max_d, max_x, max_y, beyond; } avx_diff_rec;

/* a_hwc, b_hwc: n_frames contiguous H x W x 3 uint8 frames on the device; out_hwc: n_frames frames of H x W x 3 (AVX_DIFF_MAP) or
 * H x 3W x 3 (AVX_DIFF_SIDE: A | B | map, written by the same launch); rec_dev: n_frames records on the device (8-byte aligned).
 * Asynchronous on `stream`.  1 <= n_frames <= 16, H*W < 2^32.  With d_c = |a_c - b_c| and d = max_c d_c of a pixel, G = gain and
 * K = threshold (0..254):
 *   AVX_DIFF_ABS  (G an integer 1..255): out_c = min(255, G d_c).
 *   AVX_DIFF_HEAT (G an integer 1..255): d <= K: out = (g, g, g), g = ((77 a_r + 150 a_g + 29 a_b + 128) >> 8) >> 2, a dim grey of
 *       A; d > K: out = pal(min(255, G (d - K))), pal(v) = (min(255, 3v), clamp(3v - 255, 0, 255), clamp(3v - 510, 0, 255)).
 *   AVX_DIFF_SSIM (0 < G <= 16, H >= 11 and W >= 11): the local SSIM of avx_frame_metrics_u8 (the same float32 arithmetic of a
 *       position).  Pixel (y, x) takes window position (clamp(y - 5, 0, H - 11), clamp(x - 5, 0, W - 11)); with s_c that position's
 *       SSIM in channel c, sbar = ((s_r + s_g) + s_b) / 3 and v = clamp(floor((255 G) (1 - sbar) + 0.5), 0, 255), all float32,
 *       out = pal(v).  Identical frames give an all-black map.  ssim_map_dev, when not NULL (this mode only; 4-byte aligned),
 *       receives the s_c themselves: float32 [frame][H - 10][W - 10][3].
 * The record is written in every mode: max_d the largest d of the frame, (max_x, max_y) the first pixel in raster order that
 * attains it ((0, 0) when max_d is 0), beyond the number of PIXELS with d > K (avx_frame_metrics' histogram counts samples).  Maps and
 * records are integers or fixed-order float32: a frame's output does not depend on its batch or on the run.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for a NULL buffer, n_frames outside 1..16, a bad size, mode or
 * layout, a gain outside the mode's range (or not an integer in the ABS and HEAT modes), a threshold outside 0..254, the SSIM mode
 * below 11 x 11, ssim_map_dev in another mode, and out_hwc overlapping an input; nothing is launched then. */
int avx_diff_map_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, int threshold,
                    int layout, uint8_t* out_hwc, avx_diff_rec* rec_dev, float* ssim_map_dev, void* stream);

/* Colour difference maps (csrc/delta_e.hip): how far apart, in perceptual units, the pixels of two batches of uint8
 * sRGB frames are -- CIEDE2000 (dE00) in CIELAB under D65 -- as float32 values, as a picture per frame and as a record per frame. */
enum avx_delta_e_mode { AVX_DELTA_E_HEAT = 0, AVX_DELTA_E_PLAIN = 1 };
enum avx_delta_e_layout { AVX_DELTA_E_MAP = 0, AVX_DELTA_E_SIDE = 1 };
typedef struct avx_delta_e_rec {
    uint32_t hist[256]; /* pixels with min(255, floor(2 dE)) == k: bins 0.5 wide, the last one open; sums to H*W */
    double sum;         /* the sum of the float32 dE of every pixel, in a fixed order */
    float max_de;       /* the largest dE of the frame */
    uint32_t max_x, max_y; /* the first pixel in raster order that attains it; (0, 0) when max_de is 0 */
    uint32_t beyond;    /* pixels with dE > threshold */
} avx_delta_e_rec;

/* a_hwc, b_hwc: n_frames contiguous H x W x 3 uint8 frames on the device; rec_dev: n_frames records on the device (8-byte aligned);
 * map_out: NULL (records only), or n_frames frames of H x W x 3 (AVX_DELTA_E_MAP) or H x 3W x 3 (AVX_DELTA_E_SIDE: A | B | map,
 * written by the same launch); de_out: NULL, or the float32 dE of every pixel, [frame][H][W] (4-byte aligned).  Asynchronous on
 * `stream`.  1 <= n_frames <= 16, H*W < 2^32.  All arithmetic is float32.
 * Lab of a pixel (r8, g8, b8): lin(code) is the sRGB decode of c = code / 255 -- c / 12.92 where c <= 0.04045, else
 * ((c + 0.055) / 1.055)^2.4 --, a 256-entry float32 table whose entries are the float64 values rounded once.  M' is the sRGB -> XYZ
 * (D65) matrix (0.4124564 0.3575761 0.1804375; 0.2126729 0.7151522 0.0721750; 0.0193339 0.1191920 0.9503041) with every row divided by
 * its own sum, so that white is (1, 1, 1).  With (r, g, b) = lin of the codes, t_i = g + M'_i0 (r - g) + M'_i2 (b - g) for i = X, Y,
 * Z: the form anchored on green is part of the definition -- r = g = b gives t_X = t_Y = t_Z exactly, so greys have a = b = 0
 * exactly; the plain product M' (r, g, b) leaves a share of the greys with a tiny chroma of random hue.  f(t) = cbrt(t) where
 * t > (6/29)^3, else t / (3 (6/29)^2) + 4/29;  L = 116 f_Y - 16, a = 500 (f_X - f_Y), b = 200 (f_Y - f_Z).
 * dE00 of two Lab triples: Sharma, Wu, Dalal 2005 with k_L = k_C = k_H = 1 and that paper's conventions: h' = atan2(b, a') mod 360
 * degrees and 0 where a' = b = 0; dh' = 0 where C'1 C'2 = 0, else folded into (-180, 180]; the mean hue is h'1 + h'2 where
 * C'1 C'2 = 0, (h'1 + h'2) / 2 where |h'1 - h'2| <= 180, otherwise (sum + 360) / 2 where the sum is below 360, else (sum - 360) / 2;
 * the radicand is clamped at 0 before the root.  Two pixels of equal codes give exactly 0.
 * The map, with G = gain (0 < G <= 255), T = threshold (finite, >= 0) and pal and the dim grey those of avx_diff_map_u8:
 *   AVX_DELTA_E_HEAT:  dE <= T: (g, g, g), g = ((77 a_r + 150 a_g + 29 a_b + 128) >> 8) >> 2;  dE > T: pal(v),
 *                      v = min(255, floor(G (dE - T) + 0.5)).
 *   AVX_DELTA_E_PLAIN: pal(min(255, floor(G dE + 0.5))) everywhere; identical frames give a black map.
 * The quantiser is float32 with one rounding per operation: the subtraction, the product and the sum with 0.5 are each rounded, the
 * multiply and the add are NOT fused (__fmul_rn, __fadd_rn).
 * The record is written whatever map_out is.  Counts are integers; the sum is formed from per-workgroup float64 partials (a
 * workgroup owns 4096 consecutive pixels, a thread adds its pixels in raster order) added in index order, without float atomics: a
 * frame's record, map and values do not depend on its batch, its place in the batch, the alignment of the buffers or the run.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for a NULL ctx, input or record pointer, n_frames outside 1..16,
 * a bad size, mode or layout, a gain outside (0, 255] or not finite, a negative or non-finite threshold, a misaligned rec_dev or
 * de_out, and map_out overlapping an input; nothing is launched or written then. */
int avx_delta_e_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, int mode, float gain, float threshold,
                   int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream);

/* S-CIELAB colour difference maps (csrc/scielab.hip; Zhang & Wandell 1996): avx_delta_e_u8 for a viewer at a stated
 * distance.  Both frames are filtered in an opponent colour space by the contrast sensitivity of the eye at `ppd` pixels per degree of
 * visual angle (pixels per unit length x viewing distance x tan 1 degree), and dE00 is taken per pixel on the filtered frames, so
 * that differences too fine to be resolved from there count for little.  Buffers, n_frames, mode, gain, threshold, layout, map_out,
 * rec_dev, de_out, the record, the quantiser, the palette and the errors are those of avx_delta_e_u8; the dim grey of the heat mode
 * and the A and B panels of the side layout are the unfiltered frames'.  2 <= ppd <= 128 and finite.
 * With lin the decode table of avx_delta_e_u8 and M its sRGB -> XYZ matrix: o = P M lin, P = (0.279 0.72 -0.107; -0.449 0.29 -0.077;
 * 0.086 -0.59 0.501) (luminance, red-green, blue-yellow).  Each channel is filtered by a sum of separable Gaussians given as (weight,
 * spread in degrees): luminance (0.921, 0.0283), (0.105, 0.133), (-0.108, 4.336); red-green (0.531, 0.0392), (0.330, 0.494);
 * blue-yellow (0.488, 0.0536), (0.371, 0.386); the weights of a channel are divided by their sum.  A term is g[x] g[y] with
 * g[x] = exp(-x^2 / (spread ppd)^2) on x = -R .. R, R = ceil(ppd / 2), normalised to unit sum over that support; the filtered channel
 * is sum_i w_i (g_i *x g_i *y o), rows first, the border clamped to the nearest pixel in both directions; frames smaller than the
 * support are legal.  t = diag(1 / rowsum(M)) P^-1 o_filtered, and Lab follows from t by f as in avx_delta_e_u8, the linear branch
 * also for the negative t the filters can produce; the form anchored on green does not apply.  Taps, weights, P M and P^-1 are formed
 * in float64 and rounded once to float32; the sums are float32 fused multiply-adds over the taps in index order.
 * Every pixel of either frame goes through the same operations, so a pixel whose (2R + 1)^2 neighbourhood is the same in A and B has
 * dE exactly 0, and identical frames give an all-zero record and a black PLAIN map.  As for avx_delta_e_u8, a frame's record, map and
 * values do not depend on its batch, its place in the batch, the alignment of the buffers or the run.  The workspace scratch holds 56
 * bytes per pixel of a frame pair; a batch is walked in groups of pairs, sized by H and W alone, that keep it at or below 1 GiB (one
 * pair above 19 Mpixel is walked alone and takes more).
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) as for avx_delta_e_u8, and for a ppd outside 2..128 or not finite. */
int avx_scielab_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, double ppd, int mode, float gain,
                   float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream);

/* Receptor-noise-limited colour distance maps (csrc/receptor.hip; Vorobyev & Osorio 1998): avx_delta_e_u8 with the
 * distance dS between the pixels of two batches of uint8 sRGB frames as an observer's receptor classes tell them apart, in
 * just-noticeable differences, in place of dE00.  The measure is chromatic: it says nothing about brightness.
 * The observer: K = n_receptors in 2..4 receptor classes; R = matrix, K rows of 3 (row-major; the rows beyond K are not read) on
 * linear RGB, every entry finite and >= 0 and every row sum > 0; e_i = weber[i], the Weber fraction of class i, 0.01 <= e_i <= 1;
 * eps = floor, 1e-6 <= eps <= 0.1 (1e-3 is the usual choice).
 * Each row of R is divided by its own sum in double and then rounded to float32 once (R'), so that white has catch 1 in every class:
 * von Kries adaptation to a white background, as avx_delta_e_u8 does with M'.
 * The catch of a pixel: with lin the 256-entry decode table of avx_delta_e_u8 and (r, g, b) = lin of the codes,
 * q_i = (g + R'_i0 (r - g)) + R'_i2 (b - g) in float32, one rounding per operation: the anchored form of avx_delta_e_u8, so a grey
 * has q_i = g exactly for every i.
 * The contrast of class i between pixel A and pixel B: df_i = logf((q_iA + eps) / (q_iB + eps)): two float32 sums, one float32
 * division, the library logf (not the fast intrinsic).
 * The distance:
 *   K = 2: dS = |df_1 - df_2| / sqrt(e_1^2 + e_2^2).
 *   K = 3: dS^2 = [e_1^2 (df_3 - df_2)^2 + e_2^2 (df_3 - df_1)^2 + e_3^2 (df_2 - df_1)^2] / [(e_1 e_2)^2 + (e_1 e_3)^2 + (e_2 e_3)^2].
 *   K = 4: dS^2 = [(e_1 e_2)^2 (df_4 - df_3)^2 + (e_1 e_3)^2 (df_4 - df_2)^2 + (e_1 e_4)^2 (df_3 - df_2)^2 + (e_2 e_3)^2 (df_4 - df_1)^2
 *                  + (e_2 e_4)^2 (df_3 - df_1)^2 + (e_3 e_4)^2 (df_2 - df_1)^2]
 *                 / [(e_1 e_2 e_3)^2 + (e_1 e_2 e_4)^2 + (e_1 e_3 e_4)^2 + (e_2 e_3 e_4)^2].
 * The weights of the numerator and the denominators are formed on the host in double; each weight is rounded to float32 once and the
 * denominator is passed as one float32 reciprocal (K = 2: of its root): dS = |df_1 - df_2| * rcp for K = 2, and for K = 3 and 4 the
 * numerator's terms are added in the order written, multiplied by rcp, and the root is taken (float32, one rounding each).
 * Two pixels of equal codes are 0 by definition and skip the arithmetic; any two greys give exactly 0, because their df_i are equal.
 * Everything downstream of the value is avx_delta_e_u8's, unchanged: the record (0.5-wide bins with the last one open, the float64
 * sum from per-chunk partials in index order, the largest value with its first pixel, beyond), the HEAT and PLAIN maps with the
 * unfused float32 quantiser, the dim grey of A, the MAP and SIDE layouts, the optional float32 value plane ds_out, the buffers and
 * their alignment, and the guarantee that a frame's record, map and values are bit-identical in any batch and at any alignment.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for everything avx_delta_e_u8 refuses, and for a NULL obs or one
 * of the wrong struct_size, n_receptors outside 2..4, a negative or non-finite matrix entry, a row whose sum is 0 or not finite, a
 * Weber fraction outside [0.01, 1] and a floor outside [1e-6, 0.1]; nothing is launched or written then. */
typedef struct avx_receptor_desc {
    uint32_t struct_size;  /* sizeof(avx_receptor_desc) */
    int32_t n_receptors;   /* K: 2, 3 or 4 */
    double matrix[12];     /* R, K rows of 3 on linear RGB, row-major */
    double weber[4];       /* e_i */
    double floor;          /* eps */
} avx_receptor_desc;
int avx_receptor_delta_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, const avx_receptor_desc* obs, int mode,
                          float gain, float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out, void* stream);

/* The receptor-noise-limited distance behind the observer's acuity blur (csrc/receptor_acuity.hip; AcuityView, Caves &
 * Johnsen 2018, followed by the distance above -- the first two stages of QCPA, van den Berg et al. 2020): avx_receptor_delta_u8 with
 * one more argument, sigma, the observer's acuity as the standard deviation of a Gaussian in pixels of the frames as given.  Both
 * frames are blurred in linear light before the catches are taken, so that differences too fine for the observer to resolve count
 * for little.  Buffers, n_frames (1..16), mode, gain, threshold, layout, map_out, rec_dev, ds_out, the record, the quantiser, the
 * palette and the errors are those of avx_delta_e_u8, the observer is avx_receptor_delta_u8's; the dim grey of the heat mode and the A
 * and B panels of the side layout are the unfiltered frames', as in avx_scielab_u8.  Per pixel:
 *   Decode: (r, g, b) = lin[code] with avx_delta_e_u8's 256-entry float32 table, for every pixel of A and of B.
 *   Taps: k = cvRound(8 sigma + 1) | 1 and t = cv::getGaussianKernel(k, sigma), t_i = exp(-(i - (k - 1) / 2)^2 / (2 sigma^2)) over their
 *       sum added left to right: the taps a species' own rendering uses (AVX_POST_GAUSS).  t is formed in double and rounded once to
 *       float32.  3 <= k <= AVX_MAX_KSIZE, which holds for 0.2 <= sigma <= 4; the radius is R = (k - 1) / 2 <= 16.
 *   Blur: each of the three linear planes of each side is blurred separably, rows (along x) first, then columns.  A sum over the taps
 *       is formed in index order in float32: s_0 = t_0 x_0 (one rounding), s_j = fma(t_j, x_j, s_(j-1)) -- the plain form, not OpenCV's
 *       symmetric-pair form.
 *   Border: BORDER_REFLECT_101, folded as often as needed, so that any frame size is legal: with p = 2 (n - 1) and
 *       m = ((i mod p) + p) mod p the index is m where m < n, else p - m; n = 1 gives 0.  Frames smaller than the radius, 1 x 1
 *       included, are legal.
 *   Catches: on the blurred values (r~, g~, b~) in the anchored form of avx_receptor_delta_u8: q_i = (g~ + R'_i0 (r~ - g~)) +
 *       R'_i2 (b~ - g~).
 *   Distance: df_i = logf((q_iA + eps) / (q_iB + eps)), and dS follows for K = 2, 3, 4 exactly as written for avx_receptor_delta_u8,
 *       with the same constants formed on the host in double.  There is NO "equal codes skip" rule here: the value of a pixel depends
 *       on its neighbourhood.
 * What follows from it: both sides run the same operations in the same order, so a pixel whose reflected (2R + 1)^2 neighbourhood is
 * the same in A and B is exactly 0; identical frames give an all-zero record and a black PLAIN map; any two frames of greys are exactly
 * 0 apart everywhere (the three blurred planes are equal, so every q_i = g~ and all df_i are equal).  A frame's record, map and values
 * do not depend on its batch, its place in the batch, the alignment of the buffers or the run: counts are integers, and the float64 sum
 * is formed from per-workgroup partials (a workgroup owns a 64 x 32 tile, a thread adds its pixels from the top down) added in an
 * order that is a function of H and W alone, without float atomics.  The call needs no scratch planes: 8 bytes of workspace a tile.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for everything avx_receptor_delta_u8 refuses, and for a sigma that
 * is not finite or outside [0.2, 4]; nothing is launched or written then. */
int avx_receptor_acuity_u8(avx_ctx* ctx, const uint8_t* a_hwc, const uint8_t* b_hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,
                           double sigma, int mode, float gain, float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out,
                           void* stream);

/* Receptor contrast within one frame (csrc/receptor_edges.hip; Local Edge Intensity Analysis, van den Berg et al. 2020:
 * the third stage of QCPA, behind the two above): per pixel of a batch (1..16) of uint8 sRGB H x W x 3 frames, the largest
 * receptor-noise-limited contrast between the pixel and its up to eight neighbours at distance D -- what stands out to this observer,
 * in just-noticeable differences -- as a float32 plane (ds_out), a picture (map_out: H x W x 3 per frame, the only layout) and an
 * avx_delta_e_rec per frame.  hwc, n_frames, H, W, mode (AVX_DELTA_E_HEAT / _PLAIN), gain, threshold, map_out, rec_dev, ds_out and
 * stream are avx_delta_e_u8's, with the one input in the place of A; frames of any size from 1 x 1 are legal.
 *   obs: the observer, avx_receptor_delta_u8's, unchanged: K = 2..4, the same checks, the same constants (R', the weights, rcp, eps).
 *   lum: the luminance channel, or NULL for none.  row: its sensitivity on linear RGB, entries finite and >= 0, sum > 0; the row is
 *       divided by its sum in double and rounded to float32 once (L'), like R'.  weber: its Weber fraction e_L, 0.01 <= e_L <= 1;
 *       1 / e_L is formed in double and rounded to float32 once.
 *   channel: AVX_EDGES_CHROMATIC (the colour distance dS), AVX_EDGES_ACHROMATIC (the luminance contrast dL) or AVX_EDGES_EITHER (the
 *       larger of the two); the last two need lum.
 *   sigma: the observer's acuity; 0 means no blur, otherwise finite and in [0.2, 4] exactly as in avx_receptor_acuity_u8.
 *   step: D, 1..8, the distance to the neighbours in pixels.
 * Per pixel p:
 *   Decode: (r, g, b) = lin[code] with avx_delta_e_u8's 256-entry float32 table.
 *   Blur (sigma != 0): the three linear planes are blurred exactly as avx_receptor_acuity_u8 blurs a side: the same taps
 *       (k = cvRound(8 sigma + 1) | 1, formed in double, summed left to right, rounded once), the same plain index-order sums
 *       s_0 = t_0 x_0, s_j = fma(t_j, x_j, s_(j-1)), rows then columns, the same BORDER_REFLECT_101 folded as often as needed.
 *   Catches: q_i = (g + R'_i0 (r - g)) + R'_i2 (b - g) for the K classes, and q_L the same form with L'.
 *   Logarithm, once per pixel: f_i = logf(q_i + eps) and f_L = logf(q_L + eps), the library logf.
 *   Neighbours: the offsets (+-D, 0), (0, +-D), (+-D, +-D).  A neighbour outside the frame is skipped; it is not reflected.  For a
 *       neighbour n inside the frame, df_i = f_i(p) - f_i(n), one float32 subtraction; dS(p, n) follows from the df_i by the formulas and
 *       constants of avx_receptor_delta_u8 (K = 2: |df_1 - df_2| rcp; K = 3, 4: the terms added in the written order, times rcp, then
 *       the root); dL(p, n) = |f_L(p) - f_L(n)| (1 / e_L); v(p, n) = dS, dL or fmaxf(dS, dL), by channel.
 *   Value: value(p) = the largest v(p, n) over the neighbours inside the frame; 0 where there are none (H <= D and W <= D).
 * Everything downstream of the value is avx_delta_e_u8's: the record, the HEAT and PLAIN quantiser and palette, and the dim grey of the
 * (unfiltered) input where value <= T.
 * What follows from it, and holds without tolerance:
 *   v(p, n) = v(n, p) bit for bit: every df changes sign exactly, and the forms are even in the df.
 *   A flat frame gives an all-zero record and a black PLAIN map.
 *   A frame of greys has a chromatic value of exactly 0 everywhere, with or without blur: the three blurred planes are equal, so every
 *       q_i = g~, all f_i are equal and so are all df_i.
 *   Without blur, transposing or mirroring the frame transposes or mirrors the value plane exactly: f depends on the pixel alone and
 *       the largest of a set does not depend on its order.
 *   AVX_EDGES_EITHER is the element-wise larger of the AVX_EDGES_CHROMATIC and AVX_EDGES_ACHROMATIC planes, bit for bit.
 *   A frame's record, map and values do not depend on its batch, its place in it, the alignment of its buffers or the run.  Counts are
 *       integers; there are no float atomics; the float64 sum is formed in an order that is a function of H, W and D alone: a
 *       workgroup of 256 threads works on a block of 64 x 32 pixels and owns the (64 - 2D) x (32 - 2D) pixels of its interior; block
 *       (i, j) starts at pixel (i (64 - 2D) - D, j (32 - 2D) - D), and there are ceil(W / (64 - 2D)) x ceil(H / (32 - 2D)) of them;
 *       thread t (column t & 63, rows 8 (t >> 6) .. + 7 of the block) adds its owned pixels inside the frame from the top down; a wave's
 *       64 threads are folded by halves (lane l += lane l + 32, 16, ... 1), the four waves are added in order, ((w0 + w1) + w2) + w3; the
 *       blocks' partials, in raster order of the blocks, are added as avx_delta_e_u8's are: thread t of 256 adds partials t, t + 256,
 *       ..., and the 256 are folded by halves.  8 bytes of workspace a block, no scratch planes.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for everything avx_receptor_delta_u8 refuses (there is no layout),
 * and for a lum of the wrong struct_size, a negative or non-finite row entry, a row whose sum is 0 or not finite, an e_L outside
 * [0.01, 1], a channel outside 0..2, AVX_EDGES_ACHROMATIC or _EITHER with a NULL lum, a sigma that is neither 0 nor a finite number in
 * [0.2, 4], and a step outside 1..8; nothing is launched or written then. */
enum avx_edges_channel { AVX_EDGES_CHROMATIC = 0, AVX_EDGES_ACHROMATIC = 1, AVX_EDGES_EITHER = 2 };
typedef struct avx_luminance_desc {
    uint32_t struct_size;  /* sizeof(avx_luminance_desc) */
    uint32_t reserved;     /* not read */
    double row[3];         /* the sensitivity on linear RGB */
    double weber;          /* e_L */
} avx_luminance_desc;
int avx_receptor_edges_u8(avx_ctx* ctx, const uint8_t* hwc, int n_frames, int H, int W, const avx_receptor_desc* obs, const avx_luminance_desc* lum,
                          int channel, double sigma, int step, int mode, float gain, float threshold, uint8_t* map_out, avx_delta_e_rec* rec_dev,
                          float* ds_out, void* stream);

/* avx_receptor_edges_u8 with an edge-preserving smoothing in receptor space in front of the neighbour contrasts (csrc/receptor_smooth.hip,
 * DESIGN §4.29): every pixel is averaged with the pixels of a window that look alike to the observer, `iterations` times, and the
 * edges are taken on the result.  It stands where QCPA (van den Berg et al. 2020) has its RNL ranked filter, in front of Local Edge
 * Intensity Analysis; the definition below is this project's own -- micaToolbox's weights are not restated here -- and differs from a
 * plain rank cut-off on purpose: the rank sets the bandwidth and the weights taper to zero at it, so the output is a continuous
 * function of the frame and a float32 device can be held to a float64 statement of it with no pixel exempted.
 *   Every argument of avx_receptor_edges_u8 means what it means there.
 *   smooth: radius R, 1..5; keep KEEP, finite, 0 < KEEP <= 1; iterations ITER, 0..8.  ITER = 0 launches no smoothing: the values, the map
 *       and the record are avx_receptor_edges_u8's byte for byte (the float64 sum included: the block pitch is the same).
 *   planes_out: NULL, or n_frames x P x H x W float32 ([frame][plane][H][W]) that take the smoothed planes.
 * The planes: f = the P planes of log-catches avx_receptor_edges_u8 forms per pixel (decode, blur, catches, logf(q + eps), once per
 * pixel, to the bit): the K receptor planes for AVX_EDGES_CHROMATIC, the one luminance plane for AVX_EDGES_ACHROMATIC, the K and then
 * the luminance plane for AVX_EDGES_EITHER.  v(p, n) is the pair value of the channel exactly as above.  One iteration replaces every
 * pixel p of every plane at once, reading only the planes of the iteration before:
 *   Window: W(p) = the pixels n inside the frame with |dx| <= R and |dy| <= R, p included; N = |W(p)|.  A pixel outside the frame is
 *       skipped, not reflected.
 *   Rank: m = ceil(KEEP N), formed on the host in double for every N = 1 .. 121 and passed to the kernel as a table; the device takes
 *       no ceil of its own.
 *   Bandwidth: t = the m-th smallest of { v(p, n) : n in W(p) }; the pixel's own 0 is the first.  t is exactly one of the values.
 *   Weights: h = t + t.  h = 0: w_n = 1 where v(p, n) = 0, else 0.  Otherwise rh = 1 / h (one division per pixel), u = v(p, n) rh,
 *       a = 1 - u u and w_n = a a where u < 1, else 0.  w_p = 1 always, so the sum of the weights is at least 1.
 *   Update: f'(p) = f(p) + (sum of w_n (f(n) - f(p))) / (sum of w_n), per plane: both sums start at 0 and run over the window in raster
 *       order (dy outer, dx inner), s = s + w_n (f(n) - f(p)); float32 throughout, no fused multiply-add, one division per plane and
 *       pixel.
 * After ITER iterations value(p) is the largest v(p, n) over the eight neighbours at distance D, on the smoothed planes, and the record
 * and the map follow as above.  The smoothing uses the channel of the edges, so with ITER > 0 AVX_EDGES_EITHER is no longer the
 * element-wise larger of the two single-channel results.
 * What follows from it, and holds without tolerance:
 *   Identical values are a fixed point: a flat frame keeps its planes bit for bit, its record is all zero and its PLAIN map black.
 *   A frame of greys keeps K bit-equal receptor planes through every iteration: its chromatic value stays exactly 0.
 *   Where at least m pixels of every window share the pixel's own log-catches (KEEP <= 0.5 and two flat colours with a straight seam at
 *       least R pixels from the frame's sides), t = 0, only those pixels weigh, every difference is 0 and the planes do not change.
 *   A frame's record, map, values and planes do not depend on its batch, its place in it, the alignment of its buffers or the run.
 * Launches and scratch: a batch is walked in groups of frames; a group's planes lie in the workspace twice (8 P bytes a pixel, at most
 * 40) behind the 8 bytes a block of the record's partials, and a group is as many frames as keep that at or below 1 GiB, at least one.
 * Per group: one launch forms the planes, one launch per iteration smooths them from one set into the other, one launch takes the
 * neighbour contrasts with avx_receptor_edges_u8's blocks and order of partials.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for everything avx_receptor_edges_u8 refuses, a smooth that is NULL
 * or of the wrong struct_size, a radius outside 1..5, a keep that is not finite or not in (0, 1], iterations outside 0..8, and a
 * planes_out that is not 4-byte aligned or overlaps the input; nothing is launched or written then. */
typedef struct avx_smooth_desc {
    uint32_t struct_size;  /* sizeof(avx_smooth_desc) */
    int32_t radius;        /* R */
    double keep;           /* KEEP */
    int32_t iterations;    /* ITER */
    uint32_t reserved;     /* not read */
} avx_smooth_desc;
int avx_receptor_edges_smooth_u8(avx_ctx* ctx, const uint8_t* hwc, int n_frames, int H, int W, const avx_receptor_desc* obs,
                                 const avx_luminance_desc* lum, int channel, double sigma, int step, const avx_smooth_desc* smooth, int mode,
                                 float gain, float threshold, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* ds_out, float* planes_out,
                                 void* stream);

/* dE_ITP of ITU-R BT.2124 (csrc/itp.hip): 720 x the Euclidean distance in ICtCp (BT.2100) with Ct halved, about 1 per
 * just-noticeable difference, defined for HDR and SDR light levels alike -- per pixel of two batches of frames, as float32 values, as
 * a picture and as a record per frame, which are avx_delta_e_u8's in every respect but the value.  A side is one of two kinds; any
 * mix is legal, and two HDR sides may differ in format, subsampling, range and transfer.
 *   AVX_ITP_HDR: data = n_frames payloads of avx_yuv_frame_size(pix_fmt, H, W) bytes in one of the four 10-bit formats, BT.2020
 *     non-constant-luminance Y'CbCr, limited (full_range 0) or full range, transfer AVX_TRANSFER_PQ or _HLG.  Samples, ranges and
 *     chroma are read exactly as avx_yuv_hdr_to_rgb_u8 reads them: y = (float)(Y - yo) * ys, cb = (float)(U - 512) * cs, cr likewise
 *     (yo = 64, ys = 1/876, cs = 1/896 limited; 0, 1/1023, 1/1023 full), the chroma block's samples for every pixel of the block,
 *     E'_R = clamp01(y + rv cr), E'_G = clamp01(y + (gu cb + gv cr)), E'_B = clamp01(y + bu cb) with the BT.2020 coefficients rounded
 *     once.  x = display light / 10000 nits per channel.  PQ: t = log2(E') * (float)(ln 2 / m2), h = 1 + t/6, then h = 1 + (t * (1/k)) h
 *     for k = 5, 4, 3, 2, u = -(t h) (= 1 - E'^(1/m2) by the series of expm1: |t| <= 0.09 for every code above 0),
 *     x = pw(max((1 - c1) - u, 0) * rcp((1 - c1) + c3 u), 1/m1), and 0 at E' = 0: the EOTF's p - c1 and c2 - c3 p without the
 *     cancellation that costs the plain form 6e-5 of x near the top.
 *     HLG: s = E'^2 / 3 where E' <= 1/2, else (exp2((E' - c) log2(e) / a) + b) / 12, and x = (0.1 pw((0.2627 s_R + 0.6780 s_G) +
 *     0.0593 s_B, 0.2)) * s: the OOTF at 1000 nits, gamma 1.2.  There is no tone map and no division by sdr_white.
 *   AVX_ITP_SDR: data = n_frames H x W x 3 uint8 sRGB frames with BT.709 primaries, code 255 shown at sdr_white nits: l = k lin(code)
 *     with k = (float)(sdr_white / 10000) and lin the 256-entry decode table of avx_delta_e_u8, then BT.709 -> BT.2020 primaries
 *     anchored on green, x_i = (l_G + N_i0 (l_R - l_G)) + N_i2 (l_B - l_G), N the inverse of the BT.2020 -> BT.709 matrix of
 *     avx_yuv_hdr_to_rgb_u8 formed in double and rounded once: a grey stays exactly grey.
 * pw(v, e) = exp2(e * log2(v)) on the hardware's v_exp_f32 and v_log_f32 for v > 0, and 0 otherwise; rcp is v_rcp_f32.
 * From x (BT.2020): LMS in the same anchored form, L = (x_G + (1688/4096) (x_R - x_G)) + (262/4096) (x_B - x_G), M with 683 and 462,
 * S with 99 and 3688 (the rows of the BT.2100 matrix sum to 4096).  L', M', S' are the PQ inverse EOTF in the form
 *     p = pw(v, m1);  n = (1 - c1) * (1 - p);  d = 1 + c3 * p;  s = n * rcp((d + d) - n);  z = s * s;
 *     v' = exp2(e * (s * (1 + z * (1/3 + z * (1/5 + z * (1/7 + z * (1/9))))))),  e = (float)(-2 m2 log2(e)):
 * with q = (c1 + c2 p) / (1 + c3 p), 1 - q = n / d is formed without cancellation (c1 = c3 - c2 + 1) and ln q = -2 atanh(s); the
 * plain exp2(m2 * log2(q)) multiplies the rounding of the logarithm by m2 = 78.84.  Then, with the factor 720 folded in,
 *     I* = 360 (L' + M'),  T* = kT0 (L' - M') + kT2 (S' - M'),  P* = kP0 (L' - M') + kP2 (S' - M'),
 *     kT0 = 360 * 6610/4096, kT2 = 360 * 7003/4096, kP0 = 720 * 17933/4096, kP2 = -720 * 543/4096 (each rounded once),
 * and dE_ITP = |dI*| where dT* == 0 and dP* == 0, else sqrt((dI*^2 + dT*^2) + dP*^2) with v_sqrt_f32.  All arithmetic is float32 with
 * one rounding per operation and nothing fused.
 * What follows: equal L', M', S' give T* = P* = 0 exactly, so any two achromatic pixels (an SDR grey; an HDR pixel with U = V = 512)
 * differ by exactly |I*_A - I*_B| = 720 |dI|, one float32 subtraction; a pixel whose samples are equal on two sides of one kind,
 * range and transfer (the formats may differ) is exactly 0 and skips the arithmetic.
 * sdr_white: finite and positive; it is read by SDR sides only.  n_frames, H, W, mode, gain, threshold, layout, map_out, rec_dev,
 * de_out and stream are avx_delta_e_u8's, and so are the record, the quantiser, the palette, the workgroup's 4096 consecutive pixels
 * and the order of the float64 sum: a frame's record, map and values do not depend on its batch, its place in it, or the alignment of
 * the buffers (payloads are staged in 16-byte, 8-byte or sample-sized loads, whichever the address and the length of a run admit).
 * The dim grey of the heat mode and the A and B panels of the side layout come from `panel`: n_frames H x W x 3 uint8 frames, for an
 * HDR side its tone-mapped decode (avx_yuv_hdr_to_rgb_u8); an SDR side is its own panel and its `panel` is not read.  Panels are
 * required only when map_out is given.
 * AVX_ERR_INVALID (avx_last_error starts with this function's name) for everything avx_delta_e_u8 and avx_yuv_hdr_to_rgb_u8 refuse of
 * these arguments (an HDR side above 32768 x 32768 or at an odd address included), and for a NULL side or one of the wrong
 * struct_size, a bad kind, an 8-bit format or GRAY on an HDR side, an HDR side without a panel when map_out is given, map_out
 * overlapping a side's data or panel, and a non-finite or non-positive sdr_white; nothing is launched or written then. */
enum avx_itp_kind { AVX_ITP_SDR = 0, AVX_ITP_HDR = 1 };
typedef struct avx_itp_side {
    uint32_t struct_size;  /* sizeof(avx_itp_side) */
    int32_t kind;          /* enum avx_itp_kind */
    const uint8_t* data;   /* HDR: the payloads as stored; SDR: the frames */
    const uint8_t* panel;  /* HDR, with map_out: the uint8 RGB frames the map shows; otherwise not read */
    int32_t pix_fmt;       /* HDR: enum avx_pix_fmt, a 10-bit format */
    int32_t full_range;    /* HDR: 0 limited, 1 full */
    int32_t transfer;      /* HDR: enum avx_transfer */
    int32_t reserved;      /* 0 */
} avx_itp_side;
int avx_itp_delta(avx_ctx* ctx, const avx_itp_side* a, const avx_itp_side* b, double sdr_white, int n_frames, int H, int W, int mode, float gain,
                  float threshold, int layout, uint8_t* map_out, avx_delta_e_rec* rec_dev, float* de_out, void* stream);

/* cv2.remap(src, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT, borderValue) on K float32 planes that share two
 * per-pixel float32 maps (anableps.py:217-226): coordinates quantised to 1/32 px like OpenCV. */
int avx_remap_linear_planes(avx_ctx* ctx, const float* src_planes, int K, int H, int W, const float* mapx_dev,
                            const float* mapy_dev, float* dst_planes, float border_value, void* stream);

/* cv2.Sobel(plane, CV_32F, 1,0 / 0,1, ksize=3, BORDER_REFLECT101) -> gx, gy (mantis_shrimp.py:122-131). */
int avx_sobel3_plane(avx_ctx* ctx, const float* plane, int H, int W, float* gx, float* gy, void* stream);

/* MantisShrimp.visualize (animals/mantis_shrimp.py:143-279) for one uint8 frame, all passes on the device:
 * decode -> panorama warp -> baseline encode; RGB->HSI (optionally at hsi_scale) x band windows -> safe_norm stack
 * -> P95 -> barcode tint; red kill / haze / pre-soft blur; Sobel polarisation gain; unsharp; barcode blend;
 * scanlines; peripheral blur blend; encode.  All O(bands), O(H), O(W) tables are built by the host. */
typedef struct avx_mantis_desc {
    uint32_t struct_size;
    int32_t n_bands;                   /* N <= 16 (mantis_shrimp.py:49-60: 10)                                  */
    const float* band_matrix_host;     /* N x 3: band-pass windows folded with the analytic lobes (input-channel order) */
    const float* band_lut_host;        /* N x 3: the hue LUT of :175-197                                        */
    int32_t n_wavelengths;             /* B: the per-wavelength tables below serve pixels with a negative channel (cubic
                                          overshoot), where clamp_min(0) of classic_rgb_to_hsi.py:81 is not the identity */
    const float* lobe_gains_host;      /* B x 3 lobe gains (column j multiplies input channel j)                 */
    float lobe_denom;                  /* the scalar denominator of classic_rgb_to_hsi.py:73-79 (+1e-8)          */
    const float* band_weights_host;    /* N x B band-pass weights (uv_helpers.py:125-139)                        */
    int32_t pano_new_w;                /* widened width of panorama_warp (0 / W: no warp)                        */
    int32_t hsi_small_h, hsi_small_w;  /* classic_rgb_to_hsi_scaled size (0: full resolution)                    */
    float red_keep;                    /* float32(1 - red_kill)                                                 */
    float haze, haze_keep, haze_tint[3];
    int32_t pre_soft_ksize; const double* pre_soft_taps_host;
    float cos2_global, sin2_global;    /* float32((1 - mix) * cos/sin(2 * evec_angle))                          */
    float orientation_mix, pol_linear_strength, pol_linear_gamma, pol_circular_strength;
    int32_t unsharp_ksize; const double* unsharp_taps_host; float unsharp_amount;
    float barcode_saturation, barcode_opacity, winner_take_most;
    const float* rows_host;            /* H: 0.5 + 0.5 sin(2 pi f y) (:257-258)                                  */
    float scan_row_gain; int32_t scan_ksize; const double* scan_taps_host;
    int32_t periph_ksize; const double* periph_taps_host;
    const float* xx_host; const float* yy_host; /* W, H: linspace(-1, 1) (:270-271)                              */
    float periph_radius, periph_softness;
    const float* lin_hwc_in;           /* optional (float frames): device H x W x 3 float32, already srgb_to_linear(to_float01(frame));
                                          in_hwc is ignored then                                                        */
    int32_t out_float;                 /* 1: both outputs are float32 H x W x 3 buffers holding the sRGB value (float frames) */
} avx_mantis_desc;

int avx_mantis_u8(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_baseline_hwc, uint8_t* out_hwc, int H, int W,
                  const avx_mantis_desc* desc, void* stream);
/* The same for n_frames contiguous uint8 frames (baselines and outputs contiguous too): independent frames run on up to four
 * internal streams forked from / joined into `stream` (renderers/video.py's frame loop hands the library a batch). */
int avx_mantis_u8_batch(avx_ctx* ctx, const uint8_t* in_hwc, uint8_t* out_baseline_hwc, uint8_t* out_hwc, int n_frames, int H, int W,
                        const avx_mantis_desc* desc, void* stream);

/* ---- stages of the other UV species, each on device pointers so that a species is a sequence of asynchronous
 * calls on one stream (animal-vision_amd/planevm.py) --------------------------------------------------------- */
/* Steps 1-2 shared by every UV species but HoneyBee (animals/reindeer.py:83-98, goldfish.py:100-113, ...):
 * to_float01 + srgb_to_linear, panorama_warp to pano_new_w (<= W: no warp) and the uint8 baseline
 * (baseline_hwc_out may be NULL).  lin_hwc_out: H x W x 3 float32. */
int avx_uv_front_u8(avx_ctx* ctx, const uint8_t* in_hwc, int H, int W, int pano_new_w, float* lin_hwc_out,
                    uint8_t* baseline_hwc_out, void* stream);
/* uv_helpers.panorama_warp (:84-99) of an H x W x 3 float32 image: INTER_CUBIC widen to new_w (> W), centre crop. */
int avx_panorama_warp_f32(avx_ctx* ctx, const float* src_hwc, int H, int W, int new_w, float* dst_hwc, void* stream);
/* classic_rgb_to_hsi / classic_rgb_to_hsi_scaled (uv_helpers.py:155-183) followed by N x integrate_band
 * (:142-146): H x W x 3 linear float32 -> H x W x N float32 (raw band integrals; safe_norm is the caller's). */
typedef struct avx_band_stack_desc {
    uint32_t struct_size;
    int32_t n_bands;                   /* N <= 16                                                              */
    const float* band_matrix_host;     /* N x 3 (see avx_mantis_desc)                                          */
    int32_t n_wavelengths;
    const float* lobe_gains_host;      /* B x 3                                                                */
    float lobe_denom;
    const float* band_weights_host;    /* N x B                                                                */
    int32_t small_h, small_w;          /* reduced size of the hsi_scale route (0: full resolution)             */
} avx_band_stack_desc;
int avx_band_stack(avx_ctx* ctx, const float* lin_hwc, int H, int W, const avx_band_stack_desc* desc,
                   float* stack_hwk_out, void* stream);
/* Batched forms: n_frames (<= AVX_EW_MAX_FRAMES) independent frames, frame f of every device pointer at pointer + f * its frame
 * stride (in ELEMENTS of that pointer; >= one frame).  The frame is a grid dimension: one launch where the single-frame call is one
 * launch (avx_band_stack's reduced-size route loops over the frames inside the call).  The tables are looked up once per call. */
int avx_uv_front_u8_batch(avx_ctx* ctx, const uint8_t* in_hwc, int n_frames, size_t in_frame_stride, int H, int W, int pano_new_w,
                          float* lin_hwc_out, size_t lin_frame_stride, uint8_t* baseline_hwc_out, size_t baseline_frame_stride,
                          void* stream);
int avx_band_stack_batch(avx_ctx* ctx, const float* lin_hwc, int n_frames, size_t lin_frame_stride, int H, int W,
                         const avx_band_stack_desc* desc, float* stack_hwk_out, size_t stack_frame_stride, void* stream);
/* avx_percentile with the result left on the device (one double, the float32 value NumPy would return). */
int avx_percentile_dev(avx_ctx* ctx, const float* data_dev, size_t n, double q, double* out_dev, void* stream);
/* `count` (<= 16) independent percentiles; up to four are resolved by the same three radix passes (the arrays of
 * pointers / sizes are host arrays of device pointers). */
int avx_percentiles_dev(avx_ctx* ctx, int count, const float* const* data_dev, const size_t* n, const double* q,
                        double* const* out_dev, void* stream);

/* ---- fused elementwise programs over float32 planes (csrc/ew.hip) --------------------------------------------
 * The remaining UV species (animals/reindeer.py:83-135, goldfish.py:86-180, ... ) are NumPy expression chains over
 * HxW planes.  One avx_ew_run = one launch evaluating a whole chain per pixel: a register program (32 float32
 * registers) whose LOAD/STORE touch only the planes that enter/leave the chain; frame-wide reductions (ndarray.min /
 * max / sum / mean) accumulate alongside and land in a device-side table of doubles that later programs read with
 * AVX_EW_SCALAR -- nothing visits the host.  Every instruction is one IEEE float32 operation (no fusing). */
enum { AVX_EW_MAX_INSN = 384, AVX_EW_MAX_PLANES = 24, AVX_EW_MAX_REGS = 32, AVX_EW_MAX_ACC = 16 };
enum {  /* opcodes: dst = op(a, b); imm = constant bits / plane index / scalar slot / third register of SELECT */
    AVX_EW_CONST = 1, AVX_EW_SCALAR, AVX_EW_LOAD, AVX_EW_STORE,
    AVX_EW_ADD, AVX_EW_SUB, AVX_EW_MUL, AVX_EW_DIV, AVX_EW_MIN, AVX_EW_MAX, AVX_EW_POW, AVX_EW_ATAN2,
    AVX_EW_NEG, AVX_EW_ABS, AVX_EW_SQRT, AVX_EW_EXP, AVX_EW_LOG, AVX_EW_SIN, AVX_EW_COS, AVX_EW_FLOOR, AVX_EW_CEIL,
    AVX_EW_CLIP01, AVX_EW_TANH,
    AVX_EW_LT, AVX_EW_LE, AVX_EW_GT, AVX_EW_GE, AVX_EW_EQ, AVX_EW_AND, AVX_EW_OR, AVX_EW_NOT,
    AVX_EW_SELECT,                      /* dst = a != 0 ? b : reg[imm & 0xff]  (np.where)                          */
    AVX_EW_ACCMIN, AVX_EW_ACCMAX, AVX_EW_ACCSUM   /* dst (an accumulator register) op= a                           */
};
/* Binary opcodes (ADD .. ATAN2 and LT .. OR) may take ONE operand from the instruction itself: op | AVX_EW_IMM_A:
 * a = float32(imm), op | AVX_EW_IMM_B: b = float32(imm) (the weak Python scalars of the reference's expressions).  Either
 * flag on any other opcode (the unary NEG .. TANH and NOT included), or both together, is AVX_ERR_INVALID. */
enum { AVX_EW_OPCODE_MASK = 0x3f, AVX_EW_IMM_A = 0x40, AVX_EW_IMM_B = 0x80 };
enum {  /* plane kinds: element i of the frame (i = y*W + x) is at ptr[i*stride] unless stated                    */
    AVX_EW_PLANE_F32 = 0,               /* float32, load/store (stride 3 + offset pointer = one channel of HWC)      */
    AVX_EW_PLANE_U8,                    /* uint8 -> float value of the byte, load only                              */
    AVX_EW_PLANE_U8_LUT,                /* uint8 -> srgb_to_linear(to_float01(byte)) (uv_helpers.py:15-37), load only */
    AVX_EW_PLANE_COL,                   /* float32 vector of W entries broadcast down the rows: ptr[x]              */
    AVX_EW_PLANE_ROW,                   /* float32 vector of H entries broadcast along the rows: ptr[y]             */
    AVX_EW_PLANE_U8_ENC                 /* store only: from_float01(linear_to_srgb(clip(v,0,1)), uint8) (:25-44)    */
};
enum { AVX_EW_ACC_MIN = 0, AVX_EW_ACC_MAX, AVX_EW_ACC_SUM, AVX_EW_ACC_MEAN };
typedef struct avx_ew_insn { uint8_t op, dst, a, b; uint32_t imm; } avx_ew_insn;
typedef struct avx_ew_plane { void* ptr; int32_t stride; int32_t kind; } avx_ew_plane;
typedef struct avx_ew_program {
    uint32_t struct_size;
    int32_t H, W;
    int32_t n_insn; const avx_ew_insn* insn_host;
    int32_t n_planes; const avx_ew_plane* planes_host;   /* device pointers                                          */
    int32_t n_acc; const int32_t* acc_host;              /* n_acc x {register, AVX_EW_ACC_*, scalar slot}            */
    double* scalars_dev; int32_t n_scalars;              /* the device-side scalar table                             */
} avx_ew_program;
int avx_ew_run(avx_ctx* ctx, const avx_ew_program* program, void* stream);
/* The same program over n_frames (<= AVX_EW_MAX_FRAMES) independent frames in ONE launch (the frame is a grid dimension).
 * plane_frame_stride_bytes_host: one entry per plane of the program, the byte distance from frame f to frame f + 1 of that plane; 0 for a
 * plane every frame shares (AVX_EW_PLANE_COL / _ROW vectors, constant maps; never a plane the program stores to).  Frame f reads
 * AVX_EW_SCALAR from scalars_dev + f * scalars_frame_stride (in doubles, >= n_scalars when the program has reductions) and leaves its
 * reductions there.  Each frame's reductions are bit-identical to avx_ew_run on that frame.  n_frames == 1 ignores the strides. */
enum { AVX_EW_MAX_FRAMES = 16 };
int avx_ew_run_batch(avx_ctx* ctx, const avx_ew_program* program, int n_frames, const size_t* plane_frame_stride_bytes_host,
                     size_t scalars_frame_stride, void* stream);
/* Programs whose structure was recorded when csrc/ew_gen.hip was generated (tools/gen_ew_kernels.py) run as their own straight-line
 * kernels; others are interpreted.  Returns the number of generated kernels; *hits / *misses count avx_ew_run calls of either kind. */
int avx_ew_spec_stats(unsigned long long* hits, unsigned long long* misses);

/* ---- MST++ helpers (ml/MST_plus_plus/predict_code/architecture/MST_Plus_Plus.py) ----------------------------
 * Hand-written kernels for the memory-bound parts of the forward pass; PyTorch-ROCm keeps the dense GEMMs/convs.
 * Pointers are torch tensors' data_ptr(); dtype 0 = float32, 1 = float16; all on `stream` (torch's current stream). */

/* MS_MSA :127-129 in one pass over qkv (n_pix x 3C, row-major: q | k | v): per head h (d = C/heads <= 32)
 *   gram[h][i][j] = sum_n k[n][h*d+i] * q[n][h*d+j]   (32x32 padded, float32)
 *   nq[c] = ||q[:,c]||_2, nk[c] = ||k[:,c]||_2        (what F.normalize(dim=-1) divides by) */
int avx_mst_gram(avx_ctx* ctx, const void* qkv, int dtype, size_t n_pix, int C, int heads, float* gram, float* nq, float* nk, void* stream);

/* Fused matrix-core kernels for an MSAB block (csrc/mst_mfma.hip), float16 activations, channel groups 32 wide
 * (C = 32, 64 or 128).  wpack: the weights in MFMA fragment order, built by ml/mst_plus_plus.py::pack_fragments.
 *
 * avx_mst_qkv_gram: MS_MSA to_q/to_k/to_v (MST_Plus_Plus.py:118-120) + the Gram matrix k^T q over all n_pix pixels per
 * head and the L2 norm of every q / k column (:127-129) in one pass over x (n_pix x C); only v (n_pix x C) is
 * written.  gram: heads x 32 x 32 float32 ([i][j] = k_i . q_j), nq / nk: C float32.
 *
 * avx_mst_ln_gemm_gelu: PreNorm LayerNorm (:57-65; statistics over the 31 real channels of each group) -> FeedForward's
 * first 1x1 conv (:145, C -> 4C) -> GELU (:146); out: rows x 4C float16. */
int avx_mst_qkv_gram(avx_ctx* ctx, const void* x, const void* wpack, size_t n_pix, int C, void* v_out, float* gram, float* nq, float* nk,
                     void* stream);
/* avx_mst_qkv_gram on v_mfma_f32_32x32x16_f16: the same results (products are exact, float32 sums in another order) from wpack16 =
 * ml/mst_plus_plus.py::pack_qkv16 ([3C/32 tiles][C/16 steps][64 lanes] x 8 halves; q / k tiles in natural channel order, v tiles row-permuted). */
int avx_mst_qkv_gram16(avx_ctx* ctx, const void* x, const void* wpack16, size_t n_pix, int C, void* v_out, float* gram, float* nq, float* nk,
                       void* stream);
int avx_mst_ln_gemm_gelu(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* wpack, size_t rows, int C,
                         void* out, void* stream);

/* FeedForward's depthwise 3x3 -> GELU -> second 1x1 conv (4C -> C) (:147-149) plus the block's residual (:184):
 * out = residual + gelu(dwconv3x3(hidden)) @ W2, hidden B x H x W x 4C float16 (never rewritten), residual / out
 * B x H x W x C float16 (out may alias residual).  C = 32 or 64. */
int avx_mst_dw_gemm_add(avx_ctx* ctx, const void* hidden, const float* w_c9, const void* w2pack, const void* residual, void* out, int B, int H,
                        int W, int C, void* stream);

/* uint8 RGB frame -> the output of MST_Plus_Plus.conv_in (:275) in one kernel: x = frame / 255 rounded to float16, reflect-padded by
 * (pad_top, pad_bottom, pad_left, pad_right) like predict_torch.py:171-183, 3x3 conv with zero padding, 31 channels stored 32 wide:
 * out (H + pads, W + pads, 32) float16.  w_27x32_dev: device float32 [27][32], row k = (ky * 3 + kx) * 3 + c, column = output channel. */
int avx_mst_conv_in_u8(avx_ctx* ctx, const uint8_t* frame_hwc, int H, int W, int pad_top, int pad_bottom, int pad_left, int pad_right,
                       const float* w_27x32_dev, void* out, void* stream);

/* avx_mst_conv3x3_add through an LDS halo tile (16 x 16 pixels, every input pixel fetched once): wpack16 = the nine taps' C x C
 * weights as v_mfma_f32_32x32x16_f16 A fragments ([9][2][64][8] float16, ml/mst_plus_plus.py::pack_fragments16 per tap). */
int avx_mst_conv3x3_lds(avx_ctx* ctx, const void* x, const void* wpack16, const void* add, void* out, int B, int H, int W, int C, void* stream);
/* avx_mst_conv3x3_lds with the Gram pass of the MSAB block that follows (avx_mst_qkv_gram16 with v_out = NULL on the conv's output, wqk16 = the q and k
 * tiles of pack_qkv16) as its epilogue: the output is not read again for it.  One frame (the Gram matrix is per frame). */
int avx_mst_conv3x3_lds_gram(avx_ctx* ctx, const void* x, const void* wpack16, const void* add, void* out, int H, int W, int C, const void* wqk16, float* gram,
                             float* nq, float* nk, void* stream);
/* The three consumers of conv_in's output taking the uint8 frame in its place: each equals avx_mst_conv_in_u8 followed by the entry point it is named after, bit for
 * bit, and conv_in's tensor is neither written nor read.  The frame, its pads and the 27 x 32 table are avx_mst_conv_in_u8's and are validated as there; x / out are
 * (H + pad_top + pad_bottom) x (W + pad_left + pad_right) x 32 float16, one frame per call.
 *   _cin           out = conv3x3(x) + conv_in(frame)                       (MST.mapping(fea) + x of the first stage)
 *   _spectral_cin  spectral integration of conv3x3(x) + conv_in(frame)     (conv_out + x; the crop window is given on the padded frame)
 *   _gram_cin      out = conv3x3(conv_in(frame)) and its Gram pass         (the first stage's embedding) */
int avx_mst_conv3x3_lds_cin(avx_ctx* ctx, const void* x, const void* wpack16, const uint8_t* frame_hwc, int H, int W, int pad_top, int pad_bottom, int pad_left, int pad_right,
                            const float* w_27x32_dev, void* out, void* stream);
int avx_mst_conv3x3_lds_spectral_cin(avx_ctx* ctx, const void* x, const void* wpack16, const uint8_t* frame_hwc, int H, int W, int pad_top, int pad_bottom, int pad_left,
                                     int pad_right, const float* w_27x32_dev, const float* weights_host, int crop_t, int crop_l, int Hc, int Wc, float* planes_out,
                                     void* partials_out, int* n_partials, void* stream);
int avx_mst_conv3x3_lds_gram_cin(avx_ctx* ctx, const uint8_t* frame_hwc, int H, int W, int pad_top, int pad_bottom, int pad_left, int pad_right, const float* w_27x32_dev,
                                 const void* wpack16, void* out, const void* wqk16, float* gram, float* nq, float* nk, void* stream);
/* The same for the decoder's step back to full resolution: avx_mst_convt2x2_fuse at C = 64 with the following block's Gram pass as its epilogue. */
int avx_mst_convt2x2_fuse_gram(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int H, int W, int C,
                               const void* wqk16, float* gram, float* nq, float* nk, void* stream);
/* MST.encoder_layers[i][1] at full resolution (MST_Plus_Plus.py:206-208): Conv2d(C -> 2C, 4, stride 2, padding 1, bias=False) on (B, H, W, C)
 * float16 -> (B, H/2, W/2, 2C), C = 32; wpack16 = [16 taps][2C/32][C/16] fragments (pack_fragments16 of W[:, :, ky, kx]^T). */
int avx_mst_down4x4(avx_ctx* ctx, const void* x, const void* wpack16, void* out, int B, int H, int W, int C, void* stream);

/* The tail of the first half of an MSAB block in one pass (MS_MSA :104-106, :132-137; MSAB :183):
 * out = v @ M + bias + dw3x3(gelu(dw3x3(v))) + x on (B, H, W, C) float16 tensors, C = 32 or 64, with M the per-frame C x C matrix
 * of avx_mst_attn_pack16 (so B frames must share M: the host calls it per frame).  v on the tile's 20 x 20 halo region and the
 * GELU'd first conv live in LDS; v and x are read once, out written once.  taps*_9xc: depthwise weights, float16, tap-major
 * [9][C].  out may be x, not v. */
int avx_mst_attn_pack16(avx_ctx* ctx, const float* gram, const float* nq, const float* nk, const float* rescale, const float* wproj_t, int C, void* mpack,
                        void* stream);
int avx_mst_attn_tail(avx_ctx* ctx, const void* v, const void* x, const void* mpack16, const void* taps1_9xc, const void* taps2_9xc, const float* bias,
                      void* out, int B, int H, int W, int C, void* stream);
/* The same with v = float16(x W_v^T) formed inside the kernel (wvpack16: W_v in pack_fragments16(transposed) order): v never exists in
 * HBM and avx_mst_qkv_gram may be called with v_out = NULL.  out != x. */
int avx_mst_attn_tail_x(avx_ctx* ctx, const void* x, const void* wvpack16, const void* mpack16, const void* taps1_9xc, const void* taps2_9xc,
                        const float* bias, void* out, int B, int H, int W, int C, void* stream);
/* The tail with BOTH depthwise convs of pos_emb and the projection on the matrix pipe (csrc/mst_fused.hip::k_mst_attn_tail_mx; round 3): a
 * v_mfma_f32_16x16x32_f16 result tile is 8 channels x 2 vertically adjacent rows x 16 pixels, a depthwise 3x3 conv is three MFMAs per tile
 * (dw1pack / dw2pack: ml/mst_plus_plus.py::pack_dw_mfma fragments of MS_MSA.pos_emb's two weights, :104-106), and v @ M accumulates into the
 * same registers through block-diagonal fragments (mpack_mx: avx_mst_attn_pack_mx).  v = float16(x W_v^T) is formed on the tile's halo as in
 * avx_mst_attn_tail_x.  C = 32, 64 or 128; out != x. */
int avx_mst_attn_tail_mx(avx_ctx* ctx, const void* x, const void* wvpack16, const void* mpack_mx, const void* dw1pack, const void* dw2pack,
                         const float* bias, void* out, int B, int H, int W, int C, void* stream);
/* The same with each depthwise unit as TWO matrix instructions (round 6): one dense v_mfma_f32_16x16x32_f16 for column shift 2, then one 2:4-sparse
 * v_smfmac_f32_16x16x64_f16 for shifts 0 and 1 (a row of the weight operand holds one non-zero per 8-channel K-octet).  dw1pack / dw2pack:
 * ml/mst_plus_plus.py::pack_dw_smfmac fragments, scaled as for avx_mst_attn_tail_mx.  Same result up to the summation order of the nine taps. */
int avx_mst_attn_tail_sp(avx_ctx* ctx, const void* x, const void* wvpack16, const void* mpack_mx, const void* dw1pack, const void* dw2pack,
                         const float* bias, void* out, int B, int H, int W, int C, void* stream);
/* avx_mst_attn_pack16's matrix M in the fragment order avx_mst_attn_tail_mx takes: [C/8][C/16][64][8] float16 (4 C^2 entries, half of them
 * the zeros of the block-diagonal form). */
int avx_mst_attn_pack_mx(avx_ctx* ctx, const float* gram, const float* nq, const float* nk, const float* rescale, const float* wproj_t, int C, void* mpack,
                         void* stream);


/* MST_Plus_Plus.conv_out + x (:289-292) with the spectral integration that follows it in the honeybee route (honeybee.py:126-135) as its epilogue: the cube is
 * never written.  x / add: (H, W, 32) float16; weights_host: 3 x 32 (illuminant folded in, band 31 zero); planes_out: 3 x Hc x Wc float32 of the frame cropped at
 * (crop_t, crop_l) (the predict harness pads frames to multiples of 16, predict_torch.py:171-183); partials_out: up to 3 x CUs x 3 records of 16 bytes, *n_partials
 * receives how many triples were written.  Feed both to avx_honeybee_u8 (source 2).  The planes equal avx_spectral_integrate's on the cube bit for bit. */
int avx_mst_conv3x3_lds_spectral(avx_ctx* ctx, const void* x, const void* wpack16, const void* add, int H, int W, int C, const float* weights_host, int crop_t,
                                 int crop_l, int Hc, int Wc, float* planes_out, void* partials_out, int* n_partials, void* stream);

/* The whole second half of an MSAB block in one kernel (MST_Plus_Plus.py:57-65 PreNorm, :141-158 FeedForward, :184 residual):
 * out = x + W2 gelu(dw3x3(gelu(W1 layernorm(x)))) on a (B, H, W, C) float16 tensor, C = 32 or 64 (31-channel groups stored
 * 32 wide; LayerNorm statistics over the real channels).  The 4C-channel hidden map lives in LDS only (16 x 16 pixel tiles,
 * 1-pixel halo recomputed).  w1pack / w2pack: the 1x1 convs' weights as v_mfma_f32_32x32x16_f16 A fragments
 * ([N/32][K/16][64][8] float16, ml/mst_plus_plus.py::pack_fragments16); taps_9xhid: the depthwise 3x3 weights, float16,
 * tap-major [9][4C].  out must not alias x (tiles read their neighbours' rows). */
int avx_mst_ffn_fused(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* w1pack, const void* taps_9xhid,
                      const void* w2pack, void* out, int B, int H, int W, int C, void* stream);
/* The same with the depthwise 3x3 conv (MST_Plus_Plus.py:151) on the matrix pipe: a result tile of v_mfma_f32_16x16x32_f16 is 8 channels x
 * 2 vertically adjacent output rows x 16 pixels, the K slots are 4 input rows x 3 column shifts of those 8 channels (three MFMAs per 256
 * outputs).  dwpack: the depthwise weights as A fragments, [4C/8 octets][3 shifts][64 lanes][8] float16
 * (ml/mst_plus_plus.py::pack_dw_mfma).  Same result up to the summation order of the nine taps (float32 accumulation in both). */
int avx_mst_ffn_fused_mx(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* w1pack, const void* dwpack,
                         const void* w2pack, void* out, int B, int H, int W, int C, void* stream);
/* avx_mst_ffn_fused_mx with the two-instruction depthwise unit of avx_mst_attn_tail_sp; dwpack: ml/mst_plus_plus.py::pack_dw_smfmac (same shape). */
int avx_mst_ffn_fused_sp(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* w1pack, const void* dwpack,
                         const void* w2pack, void* out, int B, int H, int W, int C, void* stream);
/* The matrix-pipe kernels evaluate GELU on PRESCALED operands (csrc/mst_common.h: x / s enters, gelu(x) / s leaves; two packed instructions fewer per pair).
 * s = avx_mst_gelu_prescale() (4: a power of two, exact in float16; 1 when the library was built without the prescaled form), and the caller scales the
 * weights around each GELU accordingly: avx_mst_ffn_fused_mx takes W1 / s in w1pack, the depthwise weights unscaled and W2 * s in w2pack -- and, since its
 * LayerNorm only centres and scales (round 3), LayerNorm's gamma and beta FOLDED into w1pack as well: row k of W1 (input channel k) times gamma[k], and row 31
 * (the first group's padding channel, whose operand the kernel sets to 1) = W1^T beta; its gamma / beta arguments are ignored;
 * avx_mst_attn_tail_mx takes pos_emb's first depthwise weights / s in dw1pack and the second * s in dw2pack. */
float avx_mst_gelu_prescale(void);

/* The order in which the persistent tile kernels of csrc/mst_fused.hip (attention tail, FeedForward, the plain 3x3 conv, the encoder's downsampling) hand the tiles
 * of a (frames x ty x tx) grid to their nwg workgroups, run on the host with the kernels' own walk (csrc/mst_tile_order.h): visit[wg * steps_cap + k] receives the
 * raster index ((frame * ty + row) * tx + column) of the tile workgroup wg takes at its k-th step, -1 past its last one; *steps_out the largest number of steps of any
 * workgroup (visit may be NULL to ask for it first).  raster = 0: the XCD-aware order -- the workgroups with the same index % 8 share one contiguous stretch of
 * the band-major order (bands of tile columns, each walked frame by frame and row by row), so neighbouring tiles meet in one L2; raster != 0: tiles wg, wg + nwg,
 * ... of the raster, which the environment variable AVX_MST_TILE_ORDER=raster (read per call) selects in the kernels.  Results do not depend on the order. */
int avx_mst_tile_order(int frames, int ty, int tx, int nwg, int raster, long long* visit, int steps_cap, int* steps_out);

/* avx_mst_ffn_fused_mx / _sp as a march down tile columns (C = 32 or 64; same weights, same results to the bit).  Tiles are 16 x 14; a workgroup walks a
 * contiguous run of the column-major tile order downwards and keeps the hidden map of a tile's two bottom halo rows on chip for the tile below, so a step runs
 * LayerNorm, the first GEMM and its GELU on 18 x 14 = 252 pixels (8 groups of 32: two items per wave) where the 16 x 16 tile's 18 x 18 halo region takes 11
 * groups (three).  At a run's first tile and at the top of a column the two rows are computed.  max_workgroups > 0 caps the grid below the launcher's own cap
 * (0: that cap), so that a few workgroups march over a small frame. */
int avx_mst_ffn_fused_mx_col(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* w1pack, const void* dwpack,
                             const void* w2pack, void* out, int B, int H, int W, int C, int max_workgroups, void* stream);
int avx_mst_ffn_fused_sp_col(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, float eps, const void* w1pack, const void* dwpack,
                             const void* w2pack, void* out, int B, int H, int W, int C, int max_workgroups, void* stream);
/* The march's tile order, run on the host with the kernel's own walk (csrc/mst_tile_order.h, ColumnWalk), as avx_mst_tile_order: workgroup wg takes the
 * positions [T r / nwg, T (r + 1) / nwg) of the column-major order (frame, tile column, tile row), r its run (the workgroups with the same index % 8 own
 * neighbouring runs).  seg[wg * steps_cap + k] (may be NULL) receives 1 where the tile starts a segment -- a run's first tile, the top of a column -- else 0. */
int avx_mst_tile_order_col(int frames, int ty, int tx, int nwg, long long* visit, unsigned char* seg, int steps_cap, int* steps_out);

/* avx_mst_attn_tail_mx / _sp as a march down tile columns (round 11; C = 32 or 64, C = 128 is refused; same arguments, same results to the bit).  Tiles are
 * 28 x 8 (C = 32: two 14-pixel column blocks) or 14 x 14 (C = 64); a workgroup walks a run of the column-major tile order downwards and keeps on chip what the
 * tile below needs of this one: its last two rows of v and of x and its last row pair of mid = gelu(dw1(v)).  A step forms v on TR x (14 TB + 4) new pixels --
 * exactly 8 groups of 32, one per wave -- and no mid row pair twice.  max_workgroups > 0 caps the grid below the launcher's own cap (0: that cap). */
int avx_mst_attn_tail_mx_col(avx_ctx* ctx, const void* x, const void* wvpack16, const void* mpack_mx, const void* dw1pack, const void* dw2pack,
                             const float* bias, void* out, int B, int H, int W, int C, int max_workgroups, void* stream);
int avx_mst_attn_tail_sp_col(avx_ctx* ctx, const void* x, const void* wvpack16, const void* mpack_mx, const void* dw1pack, const void* dw2pack,
                             const float* bias, void* out, int B, int H, int W, int C, int max_workgroups, void* stream);
/* The steps of that march, run on the host with the kernel's own walk (csrc/mst_tile_order.h, ColumnSteps): the tiles of avx_mst_tile_order_col, with a PRIMING
 * step in front of every tile that starts a segment -- the kernel's ordinary step on the tile above it (above the frame at the top of a column) without stores,
 * which leaves on chip what the segment's first tile carries in.  visit[wg * steps_cap + k]: the raster index of the tile the step belongs to, -1 past the last
 * step; prime[...] (may be NULL): 1 for a priming step (the step after it has the same visit[] entry), else 0; *steps_out: the most steps of any workgroup. */
int avx_mst_tail_march_steps(int frames, int ty, int tx, int nwg, long long* visit, unsigned char* prime, int steps_cap, int* steps_out);

/* out = [add +] a @ W [+ a2 @ W2] for (rows x C) float16 tensors and C x C weights in fragment order (out may alias
 * add; a2 / W2 and add may be NULL): MS_MSA's `proj(attn @ v)` collapsed to one matrix per frame (:132-135)
 * accumulated onto pos_emb(v) + x, and the decoder's 1x1 fusion conv over [up | skip] (:257) without the concatenation. */
int avx_mst_rowgemm_add(avx_ctx* ctx, const void* a, const void* wpack, const void* a2, const void* wpack2, const void* add, void* out, size_t rows,
                        int C, void* stream);

/* MS_MSA :127-135 after avx_mst_qkv_gram: attn = softmax over the 31 real columns of gram / (nk nq^T) * rescale per
 * head, M = blockdiag(attn_h^T) @ W_proj^T (wproj_t: C x C float32, row = input channel), written as float16 in the
 * fragment order avx_mst_rowgemm_add takes. */
int avx_mst_attn_pack(avx_ctx* ctx, const float* gram, const float* nq, const float* nk, const float* rescale, const float* wproj_t, int C,
                      void* mpack, void* stream);

/* Dense 3x3 conv, zero padding 1, C -> C on B x H x W x C float16 (C = 32), optionally + add: MST.embedding / mapping
 * (:199, :228 with its `+ x`) and conv_out (:277, :291).  wpack: 9 taps x (C x C) in fragment order. */
int avx_mst_conv3x3_add(avx_ctx* ctx, const void* x, const void* wpack, const void* add, void* out, int B, int H, int W, int C, void* stream);

/* MS_MSA's pos_emb (:104-106: depthwise 3x3 -> GELU -> depthwise 3x3) in one pass, + residual + bias[c] (both optional):
 * out = dw2(gelu(dw1(v))) + residual + bias on B x H x W x C float16 (C = 32, 64, 128); taps C x 9 float32. */
int avx_mst_posemb(avx_ctx* ctx, const void* v, const float* w1_c9, const float* w2_c9, const void* residual, const float* bias, void* out, int B,
                   int H, int W, int C, void* stream);

/* ConvTranspose2d(C -> C/2, kernel 2, stride 2) + bias on B x H x W x C float16 -> B x 2H x 2W x C/2 (MST decoder, :214,
 * :256): four independent C x C/2 products, one per output-pixel parity.  wpack: 4 taps (dy*2 + dx) in fragment order. */
int avx_mst_convt2x2(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, void* out, int B, int H, int W, int C, void* stream);
/* The same with the decoder's 1x1 fusion conv over [up | skip] (:257) folded in: wpack / bias carry the taps composed with the
 * conv's `up` half (W_tap @ W_up^T, b @ W_up^T, built by the host), `skip` is the (B, 2H, 2W, C/2) skip tensor and wskip the conv's
 * `skip` half in fragment order ([C/64][C/16][64] x 4 float16, pack_fragments(..., True)): out = convT'(x) + skip @ W_skip^T. */
int avx_mst_convt2x2_fuse(avx_ctx* ctx, const void* x, const void* wpack, const float* bias, const void* skip, const void* wskip, void* out, int B, int H,
                          int W, int C, void* stream);
/* Both of the above on v_mfma_f32_32x32x16_f16 (skip and wskip16 both NULL: the plain transposed conv): wpack16 = 4 taps x pack_fragments16(W_tap,
 * halfrow=True) ([C/64][C/16][64] x 8 float16 each), wskip16 = pack_fragments16(W_skip, halfrow=True).  Same walk, stores and roundings; a pixel's
 * products may be summed in another order than the K = 8 kernels sum them. */
int avx_mst_convt2x2_fuse16(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int B, int H,
                            int W, int C, void* stream);
/* avx_mst_convt2x2_fuse16 with the Gram pass of the MSAB block that follows as its epilogue (one frame): C = 64 (heads = 1) or 128 (heads = 2);
 * wqk16 = the block's avx_mst_qkv_gram16 weights (its q and k tiles are read); gram (heads, 32, 32), nq / nk (heads * 32) as avx_mst_qkv_gram16
 * computes them from `out`. */
int avx_mst_convt2x2_fuse16_gram(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int H, int W,
                                 int C, int heads, const void* wqk16, float* gram, float* nq, float* nk, void* stream);
/* avx_mst_convt2x2_fuse16 (skip and wskip16 given) and avx_mst_convt2x2_fuse16_gram with whole-line memory accesses: a wave-tile's skip rows come in and its
 * output rows go out as 1 KB runs through a wave-private LDS area (csrc/mst_convt_lines.h) instead of 16 bytes per lane out of every other pixel.  Same
 * arguments and validation, the same `out` to the bit; the Gram partials are summed over other workgroups (one workgroup per CU), so gram / nq / nk agree
 * with avx_mst_convt2x2_fuse16_gram's up to the order of the float32 sums. */
int avx_mst_convt2x2_fuse16_ln(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int B, int H,
                               int W, int C, void* stream);
int avx_mst_convt2x2_fuse16_gram_ln(avx_ctx* ctx, const void* x, const void* wpack16, const float* bias, const void* skip, const void* wskip16, void* out, int H,
                                    int W, int C, int heads, const void* wqk16, float* gram, float* nq, float* nk, void* stream);
/* Where that kernel's bytes sit in a wave's row area, from the kernel's own functions run on the host (C = 64 or 128; byte offsets; any array may be NULL):
 * fetch[i * 64 + l]: the byte of the row's run that lane l of 1 KB piece i fetches (it lands at area byte 1024 i + 16 l); operand[(dx * C/32 + s) * 64 + lane]:
 * the area byte lane (p, h) reads as its operand of tap dx, step s; out_write[((dx * C/64 + t) * 2 + b) * 64 + lane]: the area byte the lane writes its channels
 * 32 t + 16 h + 8 b ... + 7 of pixel 2 p + dx to; out_read[i * 64 + l]: the area byte lane l reads back for the run's byte 1024 i + 16 l. */
int avx_mst_convt_lines_map(int C, int* fetch, int* operand, int* out_write, int* out_read);

/* nn.Conv2d(C, C, 3, 1, 1, groups=C, bias=False) on a channels-last (B,H,W,C) tensor (pos_emb :104-106,
 * FeedForward :147), float32 accumulate; w_c9: C x 9 float32 (weight.reshape(C, 9)); gelu_out: exact-erf GELU. */
int avx_dwconv3x3_nhwc(avx_ctx* ctx, const void* x, const float* w_c9, void* y, int dtype, int B, int H, int W, int C, int gelu_out, void* stream);
/* The same with a fused epilogue (float16 only, C % 8 == 0): y = dwconv(x) [GELU] + residual + bias[c]; residual (same
 * shape as y) and bias (C float32) may be NULL.  MS_MSA's `out_c + pos_emb(v)` and the block's `+ x` (:137, :183). */
int avx_dwconv3x3_nhwc_add(avx_ctx* ctx, const void* x, const float* w_c9, void* y, int B, int H, int W, int C, int gelu_out,
                           const void* residual, const float* bias, void* stream);

/* nn.LayerNorm(C) (PreNorm :57-65) over the last dim of (rows x C): biased variance, float32 statistics. */
int avx_layernorm_rows(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, void* y, int dtype, size_t rows, int C, float eps, void* stream);
/* The same over channel groups stored with zero padding (MST++'s 31-channel groups kept 32 wide so that every row
 * is 64-byte aligned): channel c takes part iff (c % group) < real; padding channels are written as zero. */
int avx_layernorm_rows_grouped(avx_ctx* ctx, const void* x, const float* gamma, const float* beta, void* y, int dtype, size_t rows, int C, float eps,
                               int group, int real, void* stream);

/* The constant tables compiled into the library (reference outputs, see csrc/srgb_tables.h):
 * which = 0: 256 x f32 decode LUT; 1: 255 x f32 encode thresholds; 2: 255 x f64 encode thresholds; 3: 3 x 256 x f32 luma tables
 * (avx_luma_mode_u8; computed, not stored).
 * Copies min(capacity, size) bytes to dst_host and returns the table's size in bytes. */
int avx_get_table(int which, void* dst_host, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* AVX_H */
