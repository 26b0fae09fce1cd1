// Control-video path of the IC-LoRA pipeline (pipelines/ic_lora.py): Canny edges on uint8 frames and the uint8 -> patchified 16-bit
// operand of the VAE encoder, with their ltx2_canny_* / ltx2_frames_to_patches C entry points (declared in include/ltx2hip.h).
// Canny is integer arithmetic throughout (the definition is written out in the header); only frames_to_patches depends on LTX2_F16.
// The source-clip glue of the retake pipeline (pipelines/retake.py) lives here too: ltx2_retake_prepare (the encoded clip -> clean tokens,
// temporal mask and noised latent in one pass) and ltx2_retake_composite (the untouched frames put back, in integers), with their twins for
// the clip's sound track: ltx2_retake_prepare_audio (the audio encoder's latent) and ltx2_retake_composite_audio (fp32 waveforms).
#include <math.h>

#include "../../include/ltx2hip.h"
#include "common.h"

namespace {

// One block owns a CN_TH x CN_TW tile of one frame: 256 threads, thread t owns 8 consecutive pixels of row t / 8.
constexpr int CN_TH = LTX2_CANNY_TILE_H, CN_TW = LTX2_CANNY_TILE_W;
constexpr int CN_PX = 8;
static_assert(CN_TH * CN_TW == 256 * CN_PX && CN_TW % CN_PX == 0, "a 256-thread block covers the tile with 8 pixels per thread");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------------------------------------
// Stage 1: gray -> Sobel -> |gx| + |gy| -> non-maximum suppression -> map {0, 1 = weak, 2 = strong}.
// LDS: gray of the tile with a 2-pixel ring (replicated at the image border), mag with a 1-pixel ring (0 outside the image).
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int CN_GW = CN_TW + 4, CN_GH = CN_TH + 4, CN_MW = CN_TW + 2, CN_MH = CN_TH + 2;

__global__ __launch_bounds__(256) void canny_map_kernel(const unsigned char* __restrict__ rgb, unsigned char* __restrict__ map, int H, int W,
                                                        int low, int high) {
    __shared__ unsigned char gray[CN_GH * CN_GW];
    __shared__ unsigned short mag[CN_MH * CN_MW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * CN_TW, y0 = blockIdx.y * CN_TH;
    const long frame = (long)blockIdx.z * H * W;

    for (int i = tid; i < CN_GH * CN_GW; i += 256) {
        const int ly = i / CN_GW, lx = i - ly * CN_GW;
        const int y = clampi(y0 + ly - 2, 0, H - 1), x = clampi(x0 + lx - 2, 0, W - 1);
        const unsigned char* p = rgb + (frame + (long)y * W + x) * 3;
        gray[i] = (unsigned char)((p[0] * 9798 + p[1] * 19235 + p[2] * 3735 + 16384) >> 15);
    }
    __syncthreads();
    // gx, gy of the pixel whose gray sits at LDS (ly, lx)
    auto sobel = [&](int ly, int lx, int& gx, int& gy) {
        const unsigned char* g = gray + ly * CN_GW + lx;
        const int a = g[-CN_GW - 1], b = g[-CN_GW], c = g[-CN_GW + 1], d = g[-1], e = g[1], f = g[CN_GW - 1], h = g[CN_GW], k = g[CN_GW + 1];
        gx = (c + 2 * e + k) - (a + 2 * d + f);
        gy = (f + 2 * h + k) - (a + 2 * b + c);
    };
    for (int i = tid; i < CN_MH * CN_MW; i += 256) {
        const int ly = i / CN_MW, lx = i - ly * CN_MW;
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        int m = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            int gx, gy;
            sobel(ly + 1, lx + 1, gx, gy);
            m = abs(gx) + abs(gy);
        }
        mag[i] = (unsigned short)m;          // <= 2040
    }
    __syncthreads();
    const int ty = tid / (CN_TW / CN_PX), tx = (tid % (CN_TW / CN_PX)) * CN_PX;
    const int y = y0 + ty;
    if (y >= H) return;
#pragma unroll
    for (int j = 0; j < CN_PX; ++j) {
        const int x = x0 + tx + j;
        if (x >= W) break;
        const unsigned short* mp = mag + (ty + 1) * CN_MW + tx + j + 1;
        const int m = mp[0];
        unsigned char v = 0;
        if (m > low) {
            int gx, gy;
            sobel(ty + 2, tx + j + 2, gx, gy);
            const int ax = abs(gx), ay = abs(gy) << 15, t22 = ax * 13573;
            bool keep;
            if (ay < t22) {
                keep = m > mp[-1] && m >= mp[1];
            } else if (ay > t22 + (ax << 16)) {
                keep = m > mp[-CN_MW] && m >= mp[CN_MW];
            } else {
                const int s = (gx ^ gy) < 0 ? -1 : 1;
                keep = m > mp[-CN_MW - s] && m > mp[CN_MW + s];
            }
            if (keep) v = m > high ? 2 : 1;
        }
        map[frame + (long)y * W + x] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Stage 2: hysteresis.  `edges` is the state (0 / 255) and the result.  One pass: every block loads its tile of the state with a 1-pixel
// ring, promotes weak pixels that touch an edge pixel until the tile stops changing (a fixpoint in LDS), and stores what it promoted.
// FIRST: the state is read from the map itself (strong -> 255), nothing reads `edges`, every pixel of the tile is stored.
// Later passes read the ring from `edges` while the neighbouring blocks may be storing to it: a pixel only ever goes 0 -> 255, so a stale
// read only delays a promotion, and a block that promoted a pixel on its tile's rim raises *changed, which makes the host launch another
// pass.  A pass in which no block raises it stored nothing any ring could have missed: all rings were exact, every tile is at its
// fixpoint, so the image is.  No block waits on another.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int CN_SW = CN_TW + 2, CN_SH = CN_TH + 2;

template <bool FIRST>
__global__ __launch_bounds__(256) void canny_hysteresis_kernel(const unsigned char* __restrict__ map, unsigned char* edges, int H, int W,
                                                               int* __restrict__ changed) {
    __shared__ unsigned char st[CN_SH * CN_SW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * CN_TW, y0 = blockIdx.y * CN_TH;
    const long frame = (long)blockIdx.z * H * W;

    for (int i = tid; i < CN_SH * CN_SW; i += 256) {
        const int ly = i / CN_SW, lx = i - ly * CN_SW;
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        unsigned char v = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const long at = frame + (long)y * W + x;
            v = FIRST ? (map[at] == 2 ? 255 : 0) : edges[at];
        }
        st[i] = v;
    }
    const int ty = tid / (CN_TW / CN_PX), tx = (tid % (CN_TW / CN_PX)) * CN_PX;
    const int y = y0 + ty;
    // bit j of `weak`: pixel j is weak and not yet an edge; bit j of `got`: this pass promoted it
    unsigned weak = 0, got = 0;
    __syncthreads();
    if (y < H) {
#pragma unroll
        for (int j = 0; j < CN_PX; ++j) {
            const int x = x0 + tx + j;
            if (x < W && map[frame + (long)y * W + x] == 1 && st[(ty + 1) * CN_SW + tx + j + 1] == 0) weak |= 1u << j;
        }
    }
    auto visit = [&](int j) {
        if (!(weak >> j & 1)) return;
        // a volatile view: every neighbour byte is loaded afresh and every promotion stored at once, whatever the compiler would keep
        volatile unsigned char* s = st + (ty + 1) * CN_SW + tx + j + 1;
        if (s[-CN_SW - 1] | s[-CN_SW] | s[-CN_SW + 1] | s[-1] | s[1] | s[CN_SW - 1] | s[CN_SW] | s[CN_SW + 1]) {
            s[0] = 255;
            weak &= ~(1u << j);
            got |= 1u << j;
        }
    };
    // neighbouring threads read these bytes while they are written: 0 -> 255 only, and the barrier below orders the rounds
    int again;
    do {
        const unsigned before = weak;
#pragma unroll
        for (int j = 0; j < CN_PX; ++j) visit(j);
#pragma unroll
        for (int j = CN_PX - 2; j >= 0; --j) visit(j);
        again = __syncthreads_or(weak != before);
    } while (again);

    if (y >= H) return;
    unsigned char* out = edges + frame + (long)y * W + x0 + tx;
    if (FIRST) {
#pragma unroll
        for (int j = 0; j < CN_PX; ++j)
            if (x0 + tx + j < W) out[j] = st[(ty + 1) * CN_SW + tx + j + 1];
    } else {
#pragma unroll
        for (int j = 0; j < CN_PX; ++j)
            if (got >> j & 1) out[j] = 255;
    }
    // only a promotion on the rim of the tile can matter to another block
    const unsigned rim = (ty == 0 || ty == CN_TH - 1) ? 0xffu : ((tx == 0 ? 1u : 0u) | (tx + CN_PX == CN_TW ? 0x80u : 0u));
    if (got & rim) atomicOr(changed, 1);
}

// ------------------------------------------------------------------------------------------------------------------------------
// uint8 frames [F][H][W][Cin] -> the encoder's patchified operand [F][H/4][W/4][64]: channel (c*4 + r_w)*4 + r_h = the pixel
// (4 hq + r_h, 4 wq + r_w) of colour c as x / 127.5 - 1, channels 48..63 zero.  A block takes FP_PIX output pixels of one patch row: the 4
// source rows are contiguous byte runs (read as dwords into LDS), the output is one contiguous run of FP_PIX * 128 bytes written 16 bytes
// per lane.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int FP_PIX = 64;

template <int CIN>
__global__ __launch_bounds__(256) void frames_to_patches_kernel(const unsigned char* __restrict__ frames, bf16* __restrict__ out, int H, int W) {
    constexpr int ROW = FP_PIX * 4 * CIN;                        // bytes of one source row of a full block
    __shared__ __attribute__((aligned(16))) unsigned char src[4 * ROW];
    const int tid = threadIdx.x;
    const int wq0 = blockIdx.x * FP_PIX, hq = blockIdx.y, Wq = W >> 2;
    const int npix = min(FP_PIX, Wq - wq0);
    const int nbytes = npix * 4 * CIN;                           // a multiple of 4, and so is every row's offset (W % 4 == 0)
    const long f = blockIdx.z;
    for (int i = tid; i < 4 * (ROW / 4); i += 256) {
        const int r = i / (ROW / 4), q = i - r * (ROW / 4);
        if (q * 4 < nbytes) {
            const unsigned char* p = frames + ((f * H + hq * 4 + r) * W + (long)wq0 * 4) * CIN;
            ((unsigned*)src)[r * (ROW / 4) + q] = ((const unsigned*)p)[q];
        }
    }
    __syncthreads();
    bf16* o = out + ((f * (H >> 2) + hq) * Wq + wq0) * 64;
    for (int i = tid; i < npix * 8; i += 256) {
        const int pix = i >> 3, k = i & 7;                       // the k-th group of 8 channels: colour k / 2, r_w = 2 (k & 1) + {0, 1}, r_h 0..3
        bf16x8 v;
        if (k < 6) {
            const int c = CIN == 1 ? 0 : (k >> 1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int rw = ((k & 1) << 1) + (e >> 2), rh = e & 3;
                const float x = (float)src[rh * ROW + (pix * 4 + rw) * CIN + c];
                v[e] = f2bf(x / 127.5f - 1.0f);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = f2bf(0.f);
        }
        *(bf16x8*)(o + (long)i * 8) = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Retake: the encoder's channel-major latent [C][P] (P = F*HW positions) -> token-major clean [P][C], mask [P] (1 on the tokens of the
// latent frames [f0, f1), 0 elsewhere) and latent = noise*sm + clean*(1 - sm) with sm = mask*noise_scale: the patchify, the
// TemporalRegionMask and the GaussianNoiser of the torch path in one pass.  Every operation is rounded on its own (contract(off): hipcc
// would fuse a*b + c into an FMA, which torch's separate statements are not), so the result is theirs bit for bit.
// A block transposes a 32 x 32 tile through LDS as vae_prepare_latent_kernel does: reads run along positions, writes along channels.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retake_prepare_kernel(const float* __restrict__ encoded, const float* __restrict__ noise, int C, long P,
                                                             long tok0, long tok1, float noise_scale, float* __restrict__ clean,
                                                             float* __restrict__ mask, float* __restrict__ latent) {
    __shared__ float tile[32][33];
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 256 threads: ty 0..7
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        const long pp = p0 + tx;
        tile[k][tx] = (c < C && pp < P) ? encoded[(long)c * P + pp] : 0.f;
    }
    __syncthreads();
    if (blockIdx.y == 0 && ty == 0 && p0 + tx < P) mask[p0 + tx] = (p0 + tx >= tok0 && p0 + tx < tok1) ? 1.f : 0.f;
    for (int k = ty; k < 32; k += 8) {
        const long pp = p0 + k;
        const int c = c0 + tx;
        if (c < C && pp < P) {
            const float m = (pp >= tok0 && pp < tok1) ? 1.f : 0.f;
            const float sm = mul_rn(m, noise_scale), om = sub_rn(1.0f, sm);
            const float v = tile[tx][k];
            clean[pp * C + c] = v;
            latent[pp * C + c] = add_rn(mul_rn(noise[pp * C + c], sm), mul_rn(v, om));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Retake: out = decoded inside the pixel-frame window [p0, p1); a frame at distance d outside it (p0 - t before, t - p1 + 1 after) is
// (decoded*a + source*(R - a) + R/2) / R with R = ramp + 1, a = max(R - d, 0), in integers: a == R is decoded, a == 0 the source's bytes.
// The clip is walked as one run of bytes, 16 per lane; a vector that lies in one frame takes one weight (and loads only the clip it
// needs when that weight is R or 0), one across a frame boundary a weight per byte, and the last total % 16 bytes go one byte per lane.
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned composite_weight(long t, int p0, int p1, unsigned R) {
    if (t >= p0 && t < p1) return R;
    const long d = t < p0 ? p0 - t : t - p1 + 1;
    return d >= (long)R ? 0u : R - (unsigned)d;
}

__device__ __forceinline__ unsigned composite_byte(unsigned d, unsigned s, unsigned a, unsigned R) { return (d * a + s * (R - a) + (R >> 1)) / R; }

__device__ __forceinline__ unsigned composite_dword(unsigned d, unsigned s, unsigned a, unsigned R) {
    unsigned o = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) o |= composite_byte((d >> k) & 255u, (s >> k) & 255u, a, R) << k;
    return o;
}

__global__ __launch_bounds__(256) void retake_composite_kernel(const unsigned char* __restrict__ decoded, const unsigned char* __restrict__ source,
                                                               unsigned char* __restrict__ out, long frame_bytes, long nvec, long total, int p0,
                                                               int p1, unsigned R) {
    const long items = nvec + (total - nvec * 16);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        if (i >= nvec) {                                                  // the scalar tail
            const long b = nvec * 16 + (i - nvec);
            const unsigned a = composite_weight(b / frame_bytes, p0, p1, R);
            out[b] = a == R ? decoded[b] : (a == 0 ? source[b] : (unsigned char)composite_byte(decoded[b], source[b], a, R));
            continue;
        }
        const long b = i * 16;
        const long t_first = b / frame_bytes;
        uint4 o;
        if (b - t_first * frame_bytes + 15 < frame_bytes) {               // the whole vector lies in frame t_first
            const unsigned a = composite_weight(t_first, p0, p1, R);
            if (a == R) {
                o = *(const uint4*)(decoded + b);
            } else if (a == 0) {
                o = *(const uint4*)(source + b);
            } else {
                const uint4 d = *(const uint4*)(decoded + b), s = *(const uint4*)(source + b);
                o.x = composite_dword(d.x, s.x, a, R);
                o.y = composite_dword(d.y, s.y, a, R);
                o.z = composite_dword(d.z, s.z, a, R);
                o.w = composite_dword(d.w, s.w, a, R);
            }
        } else {                                                          // across a frame boundary: one weight per byte
            const uint4 d = *(const uint4*)(decoded + b), s = *(const uint4*)(source + b);
            const unsigned dd[4] = {d.x, d.y, d.z, d.w}, ss[4] = {s.x, s.y, s.z, s.w};
            unsigned oo[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const unsigned ak = composite_weight((b + k) / frame_bytes, p0, p1, R);
                const int sh = (k & 3) * 8;
                oo[k >> 2] |= composite_byte((dd[k >> 2] >> sh) & 255u, (ss[k >> 2] >> sh) & 255u, ak, R) << sh;
            }
            o = make_uint4(oo[0], oo[1], oo[2], oo[3]);
        }
        *(uint4*)(out + b) = o;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Retake with sound: the audio encoder's latent [C][T][M] -> token-major clean [T][C*M] (AudioPatchifier.patchify), mask [T] (1 on the
// latent frames [a0, a1)) and latent = noise*sm + clean*(1 - sm), sm = mask*noise_scale, rounded as retake_prepare_kernel rounds.  One
// lane per output element; the whole track is a few thousand floats (C*M = 128 per 40 ms), so there is no tile to stage: a row of M
// consecutive lanes reads M consecutive floats and writes M consecutive floats.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retake_prepare_audio_kernel(const float* __restrict__ encoded, const float* __restrict__ noise, int C, int T,
                                                                   int M, int a0, int a1, float noise_scale, float* __restrict__ clean,
                                                                   float* __restrict__ mask, float* __restrict__ latent) {
    const long row = (long)C * M, n = row * T;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int t = (int)(i / row), r = (int)(i - (long)t * row), c = r / M, m = r - c * M;
        const float mk = (t >= a0 && t < a1) ? 1.f : 0.f;
        const float sm = mul_rn(mk, noise_scale), om = sub_rn(1.0f, sm);
        const float v = encoded[((long)c * T + t) * M + m];
        if (r == 0) mask[t] = mk;
        clean[i] = v;
        latent[i] = add_rn(mul_rn(noise[i], sm), mul_rn(v, om));
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Retake with sound: fp32 waveforms [channels][S].  out = decoded on the samples [s0, s1); a sample at distance d outside the window (as
// composite_weight measures it) is (decoded*a + source*(R - a)) / R with R = ramp + 1, a = max(R - d, 0): two multiplies, one add and one
// IEEE divide, each rounded on its own.  a == 0 takes the source's own bits (the formula would turn a source -0.0f into +0.0f and let a
// decoded inf or NaN through a zero weight).  R <= 2^24, so (float)a and (float)(R - a) are exact.
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retake_composite_audio_kernel(const float* __restrict__ decoded, const float* __restrict__ source,
                                                                     float* __restrict__ out, long S, long total, long s0, long s1, unsigned R) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long s = i % S;
        float o;
        if (s >= s0 && s < s1) {
            o = decoded[i];
        } else {
            const long d = s < s0 ? s0 - s : s - s1 + 1;
            if (d >= (long)R) {
                o = source[i];
            } else {
                const unsigned a = R - (unsigned)d;
                o = __fdiv_rn(add_rn(mul_rn(decoded[i], (float)a), mul_rn(source[i], (float)(R - a))), (float)R);
            }
        }
        out[i] = o;
    }
}

bool ranges_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

bool canny_shape_ok(int F, int H, int W) { return F > 0 && H > 0 && W > 0 && F <= 65535 && (H + CN_TH - 1) / CN_TH <= 65535; }

}  // namespace

extern "C" {

int ltx2_canny_hysteresis(const uint8_t* map, int F, int H, int W, uint8_t* edges, void* workspace, int64_t workspace_bytes, int* passes,
                          void* stream) {
    LTX2_CHECK_ARG(map && edges && workspace, "canny_hysteresis: null operand");
    LTX2_CHECK_ARG(canny_shape_ok(F, H, W), "canny_hysteresis: F %d H %d W %d", F, H, W);
    LTX2_CHECK_ARG(workspace_bytes >= LTX2_CANNY_FLAG_BYTES && ((uintptr_t)workspace & 3) == 0,
                   "canny_hysteresis: workspace of %ld bytes (needs %d, 4-byte aligned)", (long)workspace_bytes, LTX2_CANNY_FLAG_BYTES);
    LTX2_CHECK_ARG(map != edges, "canny_hysteresis: in place is not supported (the map is read in every pass)");
    hipStream_t s = (hipStream_t)stream;
    int* flag = (int*)workspace;
    const dim3 grid((W + CN_TW - 1) / CN_TW, (H + CN_TH - 1) / CN_TH, F);
    const long cap = (long)H * W;            // a pass that raises the flag promoted at least one pixel of some frame's rim
    int n = 0;
    for (long pass = 0; pass <= cap; ++pass) {
        int host = 0;
        hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
        if (e == hipSuccess) {
            if (pass == 0)
                hipLaunchKernelGGL(canny_hysteresis_kernel<true>, grid, dim3(256), 0, s, map, edges, H, W, flag);
            else
                hipLaunchKernelGGL(canny_hysteresis_kernel<false>, grid, dim3(256), 0, s, map, edges, H, W, flag);
            LTX2_CHECK_LAUNCH("canny_hysteresis_kernel");
            e = hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            ltx2_set_error("canny_hysteresis: %s", hipGetErrorString(e));
            return LTX2_E_HIP;
        }
        ++n;
        if (!host) {
            if (passes) *passes = n;
            return LTX2_OK;
        }
    }
    ltx2_set_error("canny_hysteresis: no fixpoint after %ld passes (H * W + 1) of a %d x %d x %d map", cap + 1, F, H, W);
    return LTX2_E_STATE;
}

int ltx2_canny_u8(const uint8_t* rgb, int F, int H, int W, float low, float high, uint8_t* edges, void* workspace, int64_t workspace_bytes,
                  int* passes, void* stream) {
    LTX2_CHECK_ARG(rgb && edges && workspace, "canny_u8: null operand");
    LTX2_CHECK_ARG(canny_shape_ok(F, H, W), "canny_u8: F %d H %d W %d", F, H, W);
    const int64_t need = LTX2_CANNY_FLAG_BYTES + (int64_t)F * H * W;
    LTX2_CHECK_ARG(workspace_bytes >= need && ((uintptr_t)workspace & 3) == 0, "canny_u8: workspace of %ld bytes (needs %ld, 4-byte aligned)",
                   (long)workspace_bytes, (long)need);
    LTX2_CHECK_ARG(low == low && high == high && fabsf(low) < 1e9f && fabsf(high) < 1e9f, "canny_u8: thresholds %f %f", low, high);
    int lo = (int)floorf(low), hi = (int)floorf(high);
    if (lo > hi) {
        const int t = lo;
        lo = hi;
        hi = t;
    }
    uint8_t* map = (uint8_t*)workspace + LTX2_CANNY_FLAG_BYTES;
    hipLaunchKernelGGL(canny_map_kernel, dim3((W + CN_TW - 1) / CN_TW, (H + CN_TH - 1) / CN_TH, F), dim3(256), 0, (hipStream_t)stream, rgb, map, H,
                       W, lo, hi);
    LTX2_CHECK_LAUNCH("canny_map_kernel");
    return ltx2_canny_hysteresis(map, F, H, W, edges, workspace, LTX2_CANNY_FLAG_BYTES, passes, stream);
}

int ltx2_frames_to_patches(const uint8_t* frames, int F, int H, int W, int Cin, void* out, void* stream) {
    LTX2_CHECK_ARG(frames && out, "frames_to_patches: null operand");
    LTX2_CHECK_ARG(Cin == 1 || Cin == 3, "frames_to_patches: Cin %d (1 or 3)", Cin);
    LTX2_CHECK_ARG(F > 0 && F <= 65535 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0 && H / 4 <= 65535, "frames_to_patches: F %d H %d W %d (H, W multiples of 4)",
                   F, H, W);
    LTX2_CHECK_ARG(((uintptr_t)frames & 3) == 0 && ((uintptr_t)out & 15) == 0, "frames_to_patches: frames 4-byte and out 16-byte aligned");
    const dim3 grid((W / 4 + FP_PIX - 1) / FP_PIX, H / 4, F);
    if (Cin == 3)
        hipLaunchKernelGGL(frames_to_patches_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, frames, (bf16*)out, H, W);
    else
        hipLaunchKernelGGL(frames_to_patches_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, frames, (bf16*)out, H, W);
    LTX2_CHECK_LAUNCH("frames_to_patches_kernel");
    return LTX2_OK;
}

int ltx2_retake_prepare(const float* encoded, const float* noise, int C, int F, int H, int W, int f0, int f1, float noise_scale, float* clean,
                        float* mask, float* latent, void* stream) {
    LTX2_CHECK_ARG(encoded && noise && clean && mask && latent, "retake_prepare: null operand");
    LTX2_CHECK_ARG(C > 0 && F > 0 && H > 0 && W > 0 && (C + 31) / 32 <= 65535, "retake_prepare: C %d F %d H %d W %d", C, F, H, W);
    LTX2_CHECK_ARG(0 <= f0 && f0 <= f1 && f1 <= F, "retake_prepare: latent-frame window [%d, %d) is not within 0 <= f0 <= f1 <= F = %d", f0, f1, F);
    LTX2_CHECK_ARG(noise_scale == noise_scale && fabsf(noise_scale) <= 1e9f, "retake_prepare: noise_scale %f", noise_scale);
    const int64_t hw = (int64_t)H * W, P = hw * F;
    LTX2_CHECK_ARG((P + 31) / 32 <= 0x7fffffffLL, "retake_prepare: %ld positions", (long)P);
    const int64_t nb = P * C * (int64_t)sizeof(float), mb = P * (int64_t)sizeof(float);
    const void* ins[2] = {encoded, noise};
    void* outs[3] = {clean, mask, latent};
    const int64_t obytes[3] = {nb, mb, nb};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 2; ++i)
            LTX2_CHECK_ARG(!ranges_overlap(outs[o], obytes[o], ins[i], nb), "retake_prepare: an output overlaps an input (out of place only)");
        for (int q = o + 1; q < 3; ++q)
            LTX2_CHECK_ARG(!ranges_overlap(outs[o], obytes[o], outs[q], obytes[q]), "retake_prepare: two outputs overlap");
    }
    const dim3 grid((unsigned)((P + 31) / 32), (C + 31) / 32);
    hipLaunchKernelGGL(retake_prepare_kernel, grid, dim3(256), 0, (hipStream_t)stream, encoded, noise, C, (long)P, (long)(f0 * hw), (long)(f1 * hw),
                       noise_scale, clean, mask, latent);
    LTX2_CHECK_LAUNCH("retake_prepare_kernel");
    return LTX2_OK;
}

int ltx2_retake_composite(const uint8_t* decoded, const uint8_t* source, int T, int H, int W, int p0, int p1, int ramp, uint8_t* out, void* stream) {
    LTX2_CHECK_ARG(decoded && source && out, "retake_composite: null operand");
    LTX2_CHECK_ARG(T > 0 && H > 0 && W > 0, "retake_composite: T %d H %d W %d", T, H, W);
    LTX2_CHECK_ARG(0 <= p0 && p0 <= p1 && p1 <= T, "retake_composite: pixel-frame window [%d, %d) is not within 0 <= p0 <= p1 <= T = %d", p0, p1, T);
    LTX2_CHECK_ARG(ramp >= 0 && ramp <= LTX2_RETAKE_MAX_RAMP, "retake_composite: ramp %d (0 .. %d)", ramp, LTX2_RETAKE_MAX_RAMP);
    const int64_t frame_bytes = (int64_t)H * W * 3, total = frame_bytes * T;
    LTX2_CHECK_ARG(!ranges_overlap(out, total, decoded, total) && !ranges_overlap(out, total, source, total),
                   "retake_composite: out overlaps an input (out of place only)");
    const bool aligned = (((uintptr_t)decoded | (uintptr_t)source | (uintptr_t)out) & 15) == 0;
    const int64_t nvec = aligned ? total / 16 : 0, items = nvec + (total - nvec * 16);
    const int64_t blocks = (items + 255) / 256;
    hipLaunchKernelGGL(retake_composite_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, decoded, source,
                       out, (long)frame_bytes, (long)nvec, (long)total, p0, p1, (unsigned)(ramp + 1));
    LTX2_CHECK_LAUNCH("retake_composite_kernel");
    return LTX2_OK;
}

int ltx2_retake_prepare_audio(const float* encoded, const float* noise, int C, int T, int M, int a0, int a1, float noise_scale, float* clean,
                              float* mask, float* latent, void* stream) {
    LTX2_CHECK_ARG(encoded && noise && clean && mask && latent, "retake_prepare_audio: null operand");
    LTX2_CHECK_ARG(C > 0 && T > 0 && M > 0 && (int64_t)C * M <= 0x7fffffffLL, "retake_prepare_audio: C %d T %d M %d", C, T, M);
    LTX2_CHECK_ARG(0 <= a0 && a0 <= a1 && a1 <= T, "retake_prepare_audio: latent-frame window [%d, %d) is not within 0 <= a0 <= a1 <= T = %d", a0, a1, T);
    LTX2_CHECK_ARG(noise_scale == noise_scale && fabsf(noise_scale) <= 1e9f, "retake_prepare_audio: noise_scale %f", noise_scale);
    const int64_t n = (int64_t)C * M * T, nb = n * (int64_t)sizeof(float), mb = T * (int64_t)sizeof(float);
    const void* ins[2] = {encoded, noise};
    void* outs[3] = {clean, mask, latent};
    const int64_t obytes[3] = {nb, mb, nb};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 2; ++i)
            LTX2_CHECK_ARG(!ranges_overlap(outs[o], obytes[o], ins[i], nb), "retake_prepare_audio: an output overlaps an input (out of place only)");
        for (int q = o + 1; q < 3; ++q)
            LTX2_CHECK_ARG(!ranges_overlap(outs[o], obytes[o], outs[q], obytes[q]), "retake_prepare_audio: two outputs overlap");
    }
    hipLaunchKernelGGL(retake_prepare_audio_kernel, dim3(grid_for(n, 256, 16384)), dim3(256), 0, (hipStream_t)stream, encoded, noise, C, T, M, a0, a1,
                       noise_scale, clean, mask, latent);
    LTX2_CHECK_LAUNCH("retake_prepare_audio_kernel");
    return LTX2_OK;
}

int ltx2_retake_composite_audio(const float* decoded, const float* source, int channels, int64_t S, int64_t s0, int64_t s1, int ramp, float* out,
                                void* stream) {
    LTX2_CHECK_ARG(decoded && source && out, "retake_composite_audio: null operand");
    LTX2_CHECK_ARG(channels > 0 && S > 0 && S <= 0x7fffffffffffLL / channels, "retake_composite_audio: channels %d S %ld", channels, (long)S);
    LTX2_CHECK_ARG(0 <= s0 && s0 <= s1 && s1 <= S, "retake_composite_audio: sample window [%ld, %ld) is not within 0 <= s0 <= s1 <= S = %ld", (long)s0,
                   (long)s1, (long)S);
    LTX2_CHECK_ARG(ramp >= 0 && ramp <= LTX2_RETAKE_AUDIO_MAX_RAMP, "retake_composite_audio: ramp %d (0 .. %d)", ramp, LTX2_RETAKE_AUDIO_MAX_RAMP);
    const int64_t total = S * channels, bytes = total * (int64_t)sizeof(float);
    LTX2_CHECK_ARG(!ranges_overlap(out, bytes, decoded, bytes) && !ranges_overlap(out, bytes, source, bytes),
                   "retake_composite_audio: out overlaps an input (out of place only)");
    hipLaunchKernelGGL(retake_composite_audio_kernel, dim3(grid_for(total, 256, 16384)), dim3(256), 0, (hipStream_t)stream, decoded, source, out,
                       (long)S, (long)total, (long)s0, (long)s1, (unsigned)(ramp + 1));
    LTX2_CHECK_LAUNCH("retake_composite_audio_kernel");
    return LTX2_OK;
}

}  // extern "C"
