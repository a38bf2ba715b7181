// preprocess.hip -- depth-map preprocessing for gfx950: BilateralFilter, DepthToVbo,
// NormalsFromVbo.
//
// Reference behaviour: src/cu_bilateral.cu:13-104, src/cu_depth_tools.cu:59-78,
// src/cu_normals.cu:12-45.  New kernels: the bilateral window is served from an LDS
// tile (workgroup tile + apron, loaded once with clamped coordinates, which is exactly
// Image::GetWithClampedRange) and the (2r+1)^2 spatial weights are evaluated once per
// workgroup into LDS instead of once per tap per pixel.

#include "kfx_device.h"
#include "host_args.h"
#include "sensor_host.h"

namespace kfx {

constexpr int BIL_MAX_R = 16; // LDS path up to a 33x33 window

struct BilParams {
    const unsigned char* in;
    size_t in_pitch;
    unsigned char* out;
    size_t out_pitch;
    int w, h;       // output extent (dOut.InBounds, cu_bilateral.cu:20,66)
    int iw, ih;     // input extent used for clamping (Image.h:297-303)
    int R;
    float gs, gr;
    float minval;
    int use_minval;
};

template <typename Ti>
__device__ __forceinline__ float load_clamped(const BilParams& p, int x, int y)
{
    x = min(max(x, 0), p.iw - 1);
    y = min(max(y, 0), p.ih - 1);
    return (float)reinterpret_cast<const Ti*>(p.in + (size_t)y * p.in_pitch)[x];
}

// KernElementwiseScaleBias (cu_operations.cu:39-49), b = s*a + offset: the ONE statement behind k_scale_bias and behind the
// converting loads of the bilateral kernels' ToMetres form, so that a sensor image filtered in one launch carries the bits of
// ScaleBias followed by BilateralFilter in both numerics modes.
__device__ __forceinline__ float scale_bias(float a, float s, float offset) { return s * a + offset; }

// What a bilateral kernel makes of a loaded pixel.  AsLoaded: the image is what is filtered (BilateralFilter).  ToMetres: the image
// is in sensor units (include/kfx_sensor.h); what is filtered is scale_bias() of it, and a workgroup writes that value of its own
// output pixels (not of the apron) to the optional `metres` image (BilateralFilterDepth).
struct AsLoaded {
    __device__ __forceinline__ float operator()(float v) const { return v; }
    __device__ __forceinline__ void keep(int, int, float) const {}
};
struct ToMetres {
    unsigned char* metres;   // Image<float> of the output's size, or null
    size_t mpitch;
    float s, offset;
    __device__ __forceinline__ float operator()(float v) const { return scale_bias(v, s, offset); }
    __device__ __forceinline__ void keep(int x, int y, float m) const
    {
        if (metres) reinterpret_cast<float*>(metres + (size_t)y * mpitch)[x] = m;
    }
};

// Workgroup = TX x TY threads (256), each thread filters PY pixels of one column, so the LDS
// tile is (TX + 2R) x (TY*PY + 2R): taller tiles amortise the apron (7x7 window at TX x TY*PY =
// 32x8: 2.1 loads per output pixel, 32x32: 1.4).  Integer inputs are held as float in LDS: every
// uchar/ushort value and every difference of two is exactly representable, so (float)(p - q),
// q >= minval and w * q give the reference's results.
template <typename Ti, int TX, int TY, int PY, typename Conv>
__global__ __launch_bounds__(TX * TY) void k_bilateral(const BilParams p, const Conv conv)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NT = TX * TY;
    const int R = p.R, D = 2 * R + 1;
    const int TW = TX + 2 * R, TH = TY * PY + 2 * R;
    float* tile = lds;          // TH x TW
    float* sw = lds + TW * TH;  // D x D spatial weights
    const int tid = threadIdx.x;
    const int bx = blockIdx.x * TX, by = blockIdx.y * (TY * PY);

    for (int i = tid; i < TW * TH; i += NT) {
        const int ty = i / TW, tx = i - ty * TW;
        tile[i] = conv(load_clamped<Ti>(p, bx + tx - R, by + ty - R));
    }
    for (int i = tid; i < D * D; i += NT) {
        const int r = i / D - R, c = i % D - R;
        const float sd2 = (float)(r * r + c * c);
        sw[i] = __expf(-(sd2) / (2 * p.gs * p.gs));
    }
    __syncthreads();

    const int lx = tid % TX, ly0 = tid / TX;
    const int x = bx + lx;
    if (x >= p.w) return;
    const float inv2gr = 2 * p.gr * p.gr;
#pragma unroll
    for (int k = 0; k < PY; ++k) {
        const int ly = ly0 + k * TY; // rows of one thread are TY apart: a wave still reads whole LDS rows
        const int y = by + ly;
        if (y >= p.h) break;
        const float pc = tile[(ly + R) * TW + lx + R];
        conv.keep(x, y, pc);
        float sum = 0.f, sumw = 0.f;
        if (!p.use_minval || pc >= p.minval) {
            for (int r = 0; r < D; ++r) {
                const float* trow = tile + (ly + r) * TW + lx;
                const float* srow = sw + r * D;
                for (int c = 0; c < D; ++c) {
                    const float q = trow[c];
                    if (!p.use_minval || q >= p.minval) {
                        const float id = pc - q;
                        const float id2 = id * id;
                        const float iw = __expf(-(id2) / inv2gr);
                        const float w = srow[c] * iw;
                        sumw += w;
                        sum += w * q;
                    }
                }
            }
        }
        reinterpret_cast<float*>(p.out + (size_t)y * p.out_pitch)[x] = sum / sumw;
    }
}

// Fast-numerics variant (kfx_set_math_mode(KFX_MATH_FAST)) for a compile-time radius: the exact kernel spends most of
// its time in the correctly rounded division -(id2) / (2 gr^2) of every tap (49 per pixel at R = 3) and in a
// data-dependent branch per tap.  Here the exponent argument is id2 * (-1 / (2 gr^2)) (one reciprocal per thread:
// the argument moves by <= 1.5 ulp, far inside the accuracy of the hardware exp), validity is a select and the
// (2R+1)^2 taps are fully unrolled.  Same tile, same tap order, same hardware exp.
template <typename Ti, int R, typename Conv>
__global__ __launch_bounds__(256) void k_bilateral_fast(const BilParams p, const Conv conv)
{
    constexpr int TX = 16, TY = 16, D = 2 * R + 1, TW = TX + 2 * R, TH = TY + 2 * R;
    __shared__ float tile[TH * TW];
    __shared__ float sw[D * D];
    const int tid = threadIdx.x;
    const int bx = blockIdx.x * TX, by = blockIdx.y * TY;
    for (int i = tid; i < TW * TH; i += 256) {
        const int ty = i / TW, tx = i - ty * TW;
        tile[i] = conv(load_clamped<Ti>(p, bx + tx - R, by + ty - R));
    }
    if (tid < D * D) {
        const int r = tid / D - R, c = tid % D - R;
        sw[tid] = __expf(-((float)(r * r + c * c)) / (2 * p.gs * p.gs));
    }
    __syncthreads();
    const int lx = tid % TX, ly = tid / TX;
    const int x = bx + lx, y = by + ly;
    if (x >= p.w || y >= p.h) return;
    const float k = -1.0f / (2 * p.gr * p.gr);
    const float pc = tile[(ly + R) * TW + lx + R];
    conv.keep(x, y, pc);
    const bool check = p.use_minval != 0;
    float sum = 0.f, sumw = 0.f;
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const float q = tile[(ly + r) * TW + lx + c];
            const bool ok = !check || q >= p.minval;
            const float id = pc - q;
            const float w = sw[r * D + c] * __expf(id * id * k);
            sumw += ok ? w : 0.f;
            sum += ok ? w * q : 0.f;
        }
    if (check && !(pc >= p.minval)) sum = sumw = 0.f; // the reference skips the window: 0 / 0 = NaN
    reinterpret_cast<float*>(p.out + (size_t)y * p.out_pitch)[x] = sum / sumw;
}

// Window too large for the LDS tile: straight global gathers.
template <typename Ti, typename Conv>
__global__ __launch_bounds__(256) void k_bilateral_global(const BilParams p, const Conv conv)
{
    int x, y;
    pixel_xy(x, y);
    if (x >= p.w || y >= p.h) return;
    const float pc = conv((float)reinterpret_cast<const Ti*>(p.in + (size_t)y * p.in_pitch)[x]);
    conv.keep(x, y, pc);
    float sum = 0.f, sumw = 0.f;
    if (!p.use_minval || pc >= p.minval) {
        for (int r = -p.R; r <= p.R; ++r)
            for (int c = -p.R; c <= p.R; ++c) {
                const float q = conv(load_clamped<Ti>(p, x + c, y + r));
                if (!p.use_minval || q >= p.minval) {
                    const float sd2 = (float)(r * r + c * c);
                    const float id = pc - q;
                    const float id2 = id * id;
                    const float w = __expf(-(sd2) / (2 * p.gs * p.gs)) * __expf(-(id2) / (2 * p.gr * p.gr));
                    sumw += w;
                    sum += w * q;
                }
            }
    }
    reinterpret_cast<float*>(p.out + (size_t)y * p.out_pitch)[x] = sum / sumw;
}

// Joint ("cross") bilateral filter with an external guide image (cu_bilateral.cu:110-143): weights
// exp(-sd2 / 2gs^2) * exp(-rd2 / 2gr^2) * exp(-cd2 / 2gc^2) with cd the guide difference; sumw == 0 keeps the input.
struct GuidedParams {
    BilParams b;
    const unsigned char* guide;
    size_t gpitch;
    int gw, gh;
    float gc;
};
template <typename Tg>
__global__ __launch_bounds__(256) void k_bilateral_guided(const GuidedParams g)
{
    const BilParams& p = g.b;
    int x, y;
    pixel_xy(x, y);
    if (x >= p.w || y >= p.h) return;
    const float pv = reinterpret_cast<const float*>(p.in + (size_t)y * p.in_pitch)[x];
    const float pcv = (float)reinterpret_cast<const Tg*>(g.guide + (size_t)y * g.gpitch)[x];
    float sum = 0.f, sumw = 0.f;
    for (int r = -p.R; r <= p.R; ++r)
        for (int c = -p.R; c <= p.R; ++c) {
            const float q = load_clamped<float>(p, x + c, y + r);
            const int gx = min(max(x + c, 0), g.gw - 1), gy = min(max(y + r, 0), g.gh - 1);
            const float qc = (float)reinterpret_cast<const Tg*>(g.guide + (size_t)gy * g.gpitch)[gx];
            const float rd = pv - q, cd = pcv - qc;
            const float sd2 = (float)(r * r + c * c);
            const float rd2 = rd * rd, cd2 = cd * cd;
            const float sw = __expf(-(sd2) / (2 * p.gs * p.gs));
            const float rw = __expf(-(rd2) / (2 * p.gr * p.gr));
            const float cw = __expf(-(cd2) / (2 * g.gc * g.gc));
            const float w = sw * rw * cw;
            sumw += w;
            sum += w * q;
        }
    reinterpret_cast<float*>(p.out + (size_t)y * p.out_pitch)[x] = sumw == 0 ? pv : sum / sumw;
}

// The parameter block of the per-pixel "out <- in" operators: pixel (x, y) of the w x h launch is out's, and in covers it
struct PixOp {
    const unsigned char* in;
    size_t in_pitch;
    unsigned char* out;
    size_t out_pitch;
    int w, h;
};
template <typename T>
__device__ __forceinline__ const T* in_row(const PixOp& p, int y) { return reinterpret_cast<const T*>(p.in + (size_t)y * p.in_pitch); }
template <typename T>
__device__ __forceinline__ T* out_row(const PixOp& p, int y) { return reinterpret_cast<T*>(p.out + (size_t)y * p.out_pitch); }

// KernDepthToVbo (cu_depth_tools.cu:59-70)
template <typename Ti>
__global__ __launch_bounds__(256) void k_depth_to_vbo(const PixOp p, const Intr K, const float scale)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.w || v >= p.h) return;
    out_row<float4>(p, v)[u] = depth_vertex(K, scale * (float)in_row<Ti>(p, v)[u], u, v);
}

// KernNormalsFromVbo (cu_normals.cu:12-38)
__global__ __launch_bounds__(256) void k_normals_from_vbo(const PixOp p)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.w || v >= p.h) return;
    float4 N = make_float4(0.f, 0.f, 0.f, 0.f);
    if (u + 1 < p.w && v + 1 < p.h) N = vertex_normal(in_row<float4>(p, v)[u], in_row<float4>(p, v)[u + 1], in_row<float4>(p, v + 1)[u]);
    out_row<float4>(p, v)[u] = N;
}

// DepthToVbo<float> and NormalsFromVbo in one launch (both are latency-sized at VGA: two 4-5 us launches become one).
// A pixel's normal needs the vertices at (u+1, v) and (u, v+1); they are recomputed from the depth image with depth_vertex,
// as DepthToVbo does, so both outputs carry exactly the bits the two separate operators write.
struct VboNrmParams {
    const unsigned char* in;
    size_t in_pitch;
    unsigned char *vbo, *nrm;
    size_t vpitch, npitch;
    int w, h;
    Intr K;
    float scale;
    unsigned char* tex;   // optional: the packed texel image {nx, ny, nz, depth} the tiled SdfFuse kernels stage by LDS-DMA (fuse.hip)
    size_t tpitch;
    float* bmax;          // ... with the maxima of its 8 x 4 pixel blocks behind it (rows of bw8 floats)
    unsigned bw8;
};
__device__ __forceinline__ float4 vertex_of(const VboNrmParams& p, int u, int v)
{
    return depth_vertex(p.K, p.scale * reinterpret_cast<const float*>(p.in + (size_t)v * p.in_pitch)[u], u, v);
}
__global__ __launch_bounds__(256) void k_vbo_normals_f32(const VboNrmParams p)
{
    __shared__ float s_max[PIX_H][8];
    int u, v, lane, wv;
    pixel_xy(u, v, lane, wv);
    float d = -__builtin_inff();
    if (u < p.w && v < p.h) {
        const float4 Vc = vertex_of(p, u, v);
        reinterpret_cast<float4*>(p.vbo + (size_t)v * p.vpitch)[u] = Vc;
        float4 N = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u + 1 < p.w && v + 1 < p.h) N = vertex_normal(Vc, vertex_of(p, u + 1, v), vertex_of(p, u, v + 1));
        reinterpret_cast<float4*>(p.nrm + (size_t)v * p.npitch)[u] = N;
        if (p.tex) {   // (uniform) the texel image of this depth image and these normals: the two steps of fuse.hip's k_pack_texels
            d = reinterpret_cast<const float*>(p.in + (size_t)v * p.in_pitch)[u];
            texel_put(p.tex, p.tpitch, u, v, N, d);
        }
    }
    if (p.tex) texel_block_max(p.bmax, p.bw8, lane, wv, d, s_max);
}

// KernElementwiseScaleBias<float,Ti,float> (cu_operations.cu:39-49): b = s*a + offset; Ti = unsigned short: a sensor's 16-bit
// readings, each exactly a float
template <typename Ti>
__global__ __launch_bounds__(256) void k_scale_bias(const PixOp p, const float s, const float offset)
{
    int x, y;
    pixel_xy(x, y);
    if (x >= p.w || y >= p.h) return;
    out_row<float>(p, y)[x] = scale_bias((float)in_row<Ti>(p, y)[x], s, offset);
}

// KernBoxHalfIgnoreInvalid<float,float,float> (cu_resample.cu:89-111): box_half of each 2x2 block
__global__ __launch_bounds__(256) void k_box_half_ignore_invalid_f32(const PixOp p)
{
    int x, y;
    pixel_xy(x, y);
    if (x >= p.w || y >= p.h) return;
    const float2 t = *reinterpret_cast<const float2*>(in_row<float>(p, 2 * y) + 2 * x);
    const float2 b = *reinterpret_cast<const float2*>(in_row<float>(p, 2 * y + 1) + 2 * x);
    out_row<float>(p, y)[x] = box_half(t.x, t.y, b.x, b.y);
}

// ---- the small per-pixel tools of cu_depth_tools.h ------------------------------------------------------------
// Disp2Depth (cu_depth_tools.cu:15-23): depth = fu * baseline / disparity, NaN below the minimum disparity
__global__ __launch_bounds__(256) void k_disp2depth(const PixOp p, float fu, float baseline, float min_disp)
{
    int x, y;
    pixel_xy(x, y);
    if (x >= p.w || y >= p.h) return;
    const float d = in_row<float>(p, y)[x];
    out_row<float>(p, y)[x] = d >= min_disp ? fu * baseline / d : __builtin_nanf("");
}

// FilterBadKinectData (cu_depth_tools.cu:32-39): millimetre readings below 200 become NaN
template <typename Ti>
__global__ __launch_bounds__(256) void k_filter_bad_kinect(const PixOp p)
{
    int x, y;
    pixel_xy(x, y);
    if (x >= p.w || y >= p.h) return;
    const float z_mm = (float)in_row<Ti>(p, y)[x];
    out_row<float>(p, y)[x] = z_mm >= 200 ? z_mm : __builtin_nanf("");
}

struct ColourVboParams {
    const unsigned char* vbo;   // Image<float4>
    size_t vpitch;
    const unsigned char* rgb;   // Image<uchar3>
    size_t rpitch;
    int rw, rh;
    unsigned char* out;         // Image<uchar4>
    size_t opitch;
    int w, h;
    Pose KT;                    // KT_cd
};

// ColourVbo (cu_depth_tools.cu:86-112): project every vertex with KT_cd, bilinear RGB (rgb_bilinear), truncated to bytes
__global__ __launch_bounds__(256) void k_colour_vbo(const ColourVboParams p)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.w || v >= p.h) return;
    const float4 Pd = *(reinterpret_cast<const float4*>(p.vbo + (size_t)v * p.vpitch) + u);
    // Mat<3,4> * Mat<4,1> with w = 1: row . (x, y, z, 1), summed left to right (Mat.h operator*)
    const float k0 = p.KT.m[0] * Pd.x + p.KT.m[1] * Pd.y + p.KT.m[2] * Pd.z + p.KT.m[3] * 1.0f;
    const float k1 = p.KT.m[4] * Pd.x + p.KT.m[5] * Pd.y + p.KT.m[6] * Pd.z + p.KT.m[7] * 1.0f;
    const float k2 = p.KT.m[8] * Pd.x + p.KT.m[9] * Pd.y + p.KT.m[10] * Pd.z + p.KT.m[11] * 1.0f;
    const float pu = k0 / k2, pv = k1 / k2;
    uchar4 id = make_uchar4(0, 0, 0, 0);
    if (1.0f <= pu && pu < ((float)p.rw - 1.0f) && 1.0f <= pv && pv < ((float)p.rh - 1.0f)) {
        const V3 c = rgb_bilinear(p.rgb, p.rpitch, pu, pv);
        id = make_uchar4((unsigned char)c.x, (unsigned char)c.y, (unsigned char)c.z, 255);
    }
    *(reinterpret_cast<uchar4*>(p.out + (size_t)v * p.opitch) + u) = id;
}

// ---- TextureDepth (cu_depth_tools.cu:123-207): colour a rendered depth image from RGB keyframes ------------------
struct KeyframeView {          // ImageKeyframe<uchar3>: {ImageIntrinsics K; Mat<float,3,4> T_iw; Image<uchar3> img}
    Intr K;
    Pose T_iw;
    const unsigned char* img;  // null: slot unused (ends the list, as `kfs[k].img.ptr` does in the reference)
    size_t pitch;
    int w, h;
};
constexpr int TEX_MAX_KF = 10;
struct TextureParams {
    unsigned char* out;        // Image<float4>
    size_t opitch;
    const unsigned char *depth, *norm, *phong;   // Image<float>, Image<float4>, Image<float> (phong: multi-keyframe variant)
    size_t dpitch, npitch, ppitch;
    int w, h, nkf, single;
    Pose T_wd;
    Intr Kd;
    KeyframeView kf[TEX_MAX_KF];
};
__global__ __launch_bounds__(256) void k_texture_depth(const TextureParams p)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.w || v >= p.h) return;
    const float d = reinterpret_cast<const float*>(p.depth + (size_t)v * p.dpitch)[u];
    const float4 N_d = reinterpret_cast<const float4*>(p.norm + (size_t)v * p.npitch)[u];
    const V3 N_w = so3_mul(p.T_wd, v3(N_d.x, N_d.y, N_d.z));
    const float4 V_d = depth_vertex(p.Kd, d, u, v);   // Unproject(u, v, z)
    const V3 P_d = v3(V_d.x, V_d.y, V_d.z);
    const V3 P_w = se3_mul(p.T_wd, P_d);
    float4 out;
    if (p.single) { // one keyframe: nearest-facing test on the camera-frame normal's z (cu_depth_tools.cu:123-149)
        const KeyframeView& k = p.kf[0];
        const V3 P_kf = se3_mul(k.T_iw, P_w);
        const float pu = k.K.u0 + k.K.fu * P_kf.x / P_kf.z, pv = k.K.v0 + k.K.fv * P_kf.y / P_kf.z;
        const V3 N_c = so3_mul(k.T_iw, N_w);
        const float facing = N_c.x * 0.f + N_c.y * 0.f + N_c.z * 1.f;
        if (2.0f <= pu && pu < ((float)k.w - 2.0f) && 2.0f <= pv && pv < ((float)k.h - 2.0f) && (double)facing < -0.2) { // the literal is a double
            const V3 c = rgb_bilinear(k.img, k.pitch, pu, pv) * (1.0f / 255.0f);
            out = make_float4(c.x, c.y, c.z, 1.f);
        } else {
            out = make_float4(0.f, 0.f, 0.f, 1.f);
        }
    } else {        // up to 10 keyframes blended by the cosine to the viewing ray (:164-197)
        float w = 0.f;
        V3 color = v3(0.f, 0.f, 0.f);   // the reference leaves `color` uninitialised before accumulating; zero here
        for (int i = 0; i < p.nkf && p.kf[i].img; ++i) {
            const KeyframeView& k = p.kf[i];
            const V3 P_kf = se3_mul(k.T_iw, P_w);
            const float pu = k.K.u0 + k.K.fu * P_kf.x / P_kf.z, pv = k.K.v0 + k.K.fv * P_kf.y / P_kf.z;
            const V3 N_c = so3_mul(k.T_iw, N_w);
            const float ndot = dot(N_c, P_kf) / -length(P_kf);
            if (2.0f <= pu && pu < ((float)k.w - 2.0f) && 2.0f <= pv && pv < ((float)k.h - 2.0f) && (double)ndot > 0.1 && P_kf.z > 0.f) {
                color = color + rgb_bilinear(k.img, k.pitch, pu, pv) * (ndot / 255.0f);
                w += ndot;
            }
        }
        if (w == 0.f) {
            w = 1.f;
            const float ph = reinterpret_cast<const float*>(p.phong + (size_t)v * p.ppitch)[u];
            color = v3(ph, ph, ph);
        }
        const V3 c = div_s(color, w);
        out = make_float4(c.x, c.y, c.z, 1.f);
    }
    reinterpret_cast<float4*>(p.out + (size_t)v * p.opitch)[u] = out;
}

} // namespace kfx

using namespace kfx;

// the parameter block of every bilateral kernel (the guided one's head included): the launch is out's, clamping is by in's extent
static BilParams bil_params(const kfx_image* out, const kfx_image* in, float gs, float gr, unsigned size, float minval, int use_minval)
{
    return BilParams{(const unsigned char*)in->ptr, in->pitch, (unsigned char*)out->ptr, out->pitch, (int)out->w, (int)out->h,
                     (int)in->w, (int)in->h, (int)size, gs, gr, minval, use_minval};
}

// tile shape of the LDS kernel (config C3 sweep, scripts/config_sweep.py): KFX_BILATERAL_TILE = 0..5, read once per process
static int bilateral_tile_shape()
{
    static const int shape = env_int("KFX_BILATERAL_TILE", 2);
    return shape;
}
template <typename Ti, int TX, int TY, int PY, typename Conv>
static void bilateral_tile_launch(const BilParams& p, const Conv& conv, hipStream_t s)
{
    const int D = 2 * p.R + 1;
    const size_t lds = (size_t)((TX + 2 * p.R) * (TY * PY + 2 * p.R) + D * D) * sizeof(float);
    hipLaunchKernelGGL((k_bilateral<Ti, TX, TY, PY, Conv>), dim3(ceil_div(p.w, TX), ceil_div(p.h, TY * PY)), dim3(TX * TY), lds, s, p, conv);
}

// The one choice of kernel, grid and LDS size behind BilateralFilter (Conv = AsLoaded) and BilateralFilterDepth (Conv = ToMetres):
// the fast kernel in fast numerics up to a 7 x 7 window, the LDS tile up to BIL_MAX_R, global gathers beyond
template <typename Ti, typename Conv>
static void bilateral_dispatch(const BilParams& p, const Conv& conv, hipStream_t s)
{
    if (math_mode() == KFX_MATH_FAST && p.R >= 1 && p.R <= 3) {
        dim3 grid(ceil_div(p.w, 16), ceil_div(p.h, 16));
        if (p.R == 3) hipLaunchKernelGGL((k_bilateral_fast<Ti, 3, Conv>), grid, dim3(256), 0, s, p, conv);
        else if (p.R == 2) hipLaunchKernelGGL((k_bilateral_fast<Ti, 2, Conv>), grid, dim3(256), 0, s, p, conv);
        else hipLaunchKernelGGL((k_bilateral_fast<Ti, 1, Conv>), grid, dim3(256), 0, s, p, conv);
    } else if (p.R <= BIL_MAX_R) {
        switch (bilateral_tile_shape()) {
        case 0: bilateral_tile_launch<Ti, 32, 8, 1>(p, conv, s); break;
        case 1: bilateral_tile_launch<Ti, 64, 4, 1>(p, conv, s); break;
        case 3: bilateral_tile_launch<Ti, 32, 8, 2>(p, conv, s); break;
        case 4: bilateral_tile_launch<Ti, 32, 8, 4>(p, conv, s); break;
        case 5: bilateral_tile_launch<Ti, 64, 4, 4>(p, conv, s); break;
        default: bilateral_tile_launch<Ti, 16, 16, 1>(p, conv, s); break; // best of the sweep at 1280x960 (profiles/r01_config_sweep.txt)
        }
    } else {
        hipLaunchKernelGGL((k_bilateral_global<Ti, Conv>), pixel_grid(p.w, p.h), dim3(256), 0, s, p, conv);
    }
}

template <typename Ti>
static int bilateral_launch(const kfx_image* out, const kfx_image* in, float gs, float gr, unsigned size,
                            float minval, int use_minval, kfx_stream stream)
{
    if (int e = check_image(out, 4, 0, 0, "BilateralFilter: output image")) return e;
    if (int e = check_image(in, sizeof(Ti), cover_w(out), cover_h(out), "BilateralFilter: input image")) return e;
    if (out->w == 0 || out->h == 0) return 0;
    if (size > 1024) return set_error(KFX_E_RANGE, "BilateralFilter: window radius");
    bilateral_dispatch<Ti>(bil_params(out, in, gs, gr, size, minval, use_minval), AsLoaded{}, (hipStream_t)stream);
    return check_launch("kfx_bilateral");
}

// BilateralFilter of a sensor image (include/kfx_sensor.h): bilateral_dispatch with the ToMetres conversion.
// launch = false: the argument checks alone (the upload ring consumes an image only once they pass).
template <typename Ti>
static int bilateral_depth_launch(const kfx_image* out, const kfx_image* metres, const kfx_image* in, float s, float offset, float gs, float gr,
                                  unsigned size, float minval, bool launch, kfx_stream stream)
{
    if (int e = check_image(out, 4, 0, 0, "BilateralFilterDepth: filtered image")) return e;
    if (metres) { if (int e = check_image(metres, 4, cover_w(out), cover_h(out), "BilateralFilterDepth: metres image")) return e; }
    if (int e = check_image(in, sizeof(Ti), cover_w(out), cover_h(out), "BilateralFilterDepth: sensor image")) return e;
    if (out->w == 0 || out->h == 0) return 0;
    if (size > 1024) return set_error(KFX_E_RANGE, "BilateralFilterDepth: window radius");
    if (!launch) return 0;
    const ToMetres conv{metres ? (unsigned char*)metres->ptr : nullptr, metres ? metres->pitch : 0, s, offset};
    bilateral_dispatch<Ti>(bil_params(out, in, gs, gr, size, minval, 1), conv, (hipStream_t)stream);
    return check_launch("kfx_bilateral_depth");
}

int kfx::bilateral_depth(const kfx_image* filtered, const kfx_image* metres, const kfx_image* raw, int format, float s, float offset, float gs,
                         float gr, unsigned size, float minval, bool launch, kfx_stream stream)
{
    if (format == KFX_DEPTH_U16) return bilateral_depth_launch<unsigned short>(filtered, metres, raw, s, offset, gs, gr, size, minval, launch, stream);
    if (format == KFX_DEPTH_F32) return bilateral_depth_launch<float>(filtered, metres, raw, s, offset, gs, gr, size, minval, launch, stream);
    return set_error(KFX_E_RANGE, "BilateralFilterDepth: format is KFX_DEPTH_U16 or KFX_DEPTH_F32");
}

// BilateralFilter(filtered, s * raw + offset, gs, gr, size, minval) with the converted image kept in `metres` (may be null)
extern "C" int kfx_bilateral_depth(const kfx_image* filtered, const kfx_image* metres, const kfx_image* raw, int format, float s, float offset,
                                   float gs, float gr, unsigned size, float minval, kfx_stream stream)
{
    return kfx::bilateral_depth(filtered, metres, raw, format, s, offset, gs, gr, size, minval, true, stream);
}

extern "C" int kfx_bilateral_f32(const kfx_image* out, const kfx_image* in, float gs, float gr, unsigned size,
                                 float minval, int use_minval, kfx_stream stream)
{
    return bilateral_launch<float>(out, in, gs, gr, size, minval, use_minval ? 1 : 0, stream);
}
extern "C" int kfx_bilateral_u16(const kfx_image* out, const kfx_image* in, float gs, float gr, unsigned size,
                                 unsigned short minval, kfx_stream stream)
{
    return bilateral_launch<unsigned short>(out, in, gs, gr, size, (float)minval, 1, stream);
}
extern "C" int kfx_bilateral_u8(const kfx_image* out, const kfx_image* in, float gs, float gr, unsigned size,
                                kfx_stream stream)
{
    return bilateral_launch<unsigned char>(out, in, gs, gr, size, 0.f, 0, stream);
}

// The preamble of the per-pixel "out <- in" entry points: out usable (out_elem-byte pixels), in usable (in_elem-byte pixels) and
// covering scale_x x scale_y times the launch; then `p` is the launch's block, and empty(p) says that there is nothing to launch --
// which the entry point answers with 0 after the checks of its other arguments.
static int pix_op(PixOp& p, const kfx_image* out, size_t out_elem, const kfx_image* in, size_t in_elem, size_t scale_x, size_t scale_y,
                  const char* what_out, const char* what_in)
{
    if (int e = check_image(out, out_elem, 0, 0, what_out)) return e;
    if (int e = check_image(in, in_elem, scale_x * cover_w(out), scale_y * cover_h(out), what_in)) return e;
    p = PixOp{(const unsigned char*)in->ptr, in->pitch, (unsigned char*)out->ptr, out->pitch, (int)out->w, (int)out->h};
    return 0;
}
static bool empty(const PixOp& p) { return p.w == 0 || p.h == 0; }

template <typename Ti>
static int vbo_launch(const kfx_image* vbo, const kfx_image* depth, const float K[4], float scale, kfx_stream stream)
{
    PixOp p;
    if (int e = pix_op(p, vbo, 16, depth, sizeof(Ti), 1, 1, "DepthToVbo: vbo image", "DepthToVbo: depth image")) return e;
    if (!K) return set_error(KFX_E_NULL, "DepthToVbo: null intrinsics");
    if (empty(p)) return 0;
    hipLaunchKernelGGL(k_depth_to_vbo<Ti>, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p, Intr{K[0], K[1], K[2], K[3]}, scale);
    return check_launch("kfx_depth_to_vbo");
}

extern "C" int kfx_depth_to_vbo_f32(const kfx_image* vbo, const kfx_image* depth, const float K[4], float scale,
                                    kfx_stream stream)
{
    return vbo_launch<float>(vbo, depth, K, scale, stream);
}
extern "C" int kfx_depth_to_vbo_u16(const kfx_image* vbo, const kfx_image* depth, const float K[4], float scale,
                                    kfx_stream stream)
{
    return vbo_launch<unsigned short>(vbo, depth, K, scale, stream);
}

extern "C" int kfx_normals_from_vbo(const kfx_image* nrm, const kfx_image* vbo, kfx_stream stream)
{
    PixOp p;
    if (int e = pix_op(p, nrm, 16, vbo, 16, 1, 1, "NormalsFromVbo: normal image", "NormalsFromVbo: vbo image")) return e;
    if (empty(p)) return 0;
    hipLaunchKernelGGL(k_normals_from_vbo, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_normals_from_vbo");
}

// ElementwiseScaleBias<float, Ti, float> (cu_operations.cu:39-57), float and unsigned short input
template <typename Ti>
static int scale_bias_launch(const kfx_image* out, const kfx_image* in, float s, float offset, const char* name, kfx_stream stream)
{
    PixOp p;
    if (int e = pix_op(p, out, 4, in, sizeof(Ti), 1, 1, "ElementwiseScaleBias: output image", "ElementwiseScaleBias: input image")) return e;
    if (empty(p)) return 0;
    hipLaunchKernelGGL(k_scale_bias<Ti>, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p, s, offset);
    return check_launch(name);
}
extern "C" int kfx_elementwise_scale_bias_f32(const kfx_image* out, const kfx_image* in, float s, float offset, kfx_stream stream)
{
    return scale_bias_launch<float>(out, in, s, offset, "kfx_elementwise_scale_bias_f32", stream);
}
extern "C" int kfx_elementwise_scale_bias_u16(const kfx_image* out, const kfx_image* in, float s, float offset, kfx_stream stream)
{
    return scale_bias_launch<unsigned short>(out, in, s, offset, "kfx_elementwise_scale_bias_u16", stream);
}

extern "C" int kfx_box_half_ignore_invalid_f32(const kfx_image* out, const kfx_image* in, kfx_stream stream)
{
    PixOp p;
    if (int e = pix_op(p, out, 4, in, 4, 2, 2, "BoxHalfIgnoreInvalid: output image", "BoxHalfIgnoreInvalid: input image (2x the output)")) return e;
    if (empty(p)) return 0;
    if (((uintptr_t)in->ptr | in->pitch) & 7) return set_error(KFX_E_ALIGN, "BoxHalfIgnoreInvalid: input not 8-byte aligned");
    hipLaunchKernelGGL(k_box_half_ignore_invalid_f32, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_box_half_ignore_invalid_f32");
}

// Disp2Depth(dIn, dOut, fu, fBaseline, fMinDisp) (cu_depth_tools.cu:15-30; the launch is bounded by dOut)
extern "C" int kfx_disp2depth(const kfx_image* in, const kfx_image* out, float fu, float baseline, float min_disp, kfx_stream stream)
{
    PixOp p;
    if (int e = pix_op(p, out, 4, in, 4, 1, 1, "Disp2Depth: output image", "Disp2Depth: input image")) return e;
    if (empty(p)) return 0;
    hipLaunchKernelGGL(k_disp2depth, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p, fu, baseline, min_disp);
    return check_launch("kfx_disp2depth");
}

// FilterBadKinectData(dFiltered, dKinectDepth) (cu_depth_tools.cu:32-53), float and unsigned short readings
template <typename Ti>
static int filter_bad_kinect_launch(const kfx_image* out, const kfx_image* in, const char* name, kfx_stream stream)
{
    PixOp p;
    if (int e = pix_op(p, out, 4, in, sizeof(Ti), 1, 1, "FilterBadKinectData: output image", "FilterBadKinectData: input image")) return e;
    if (empty(p)) return 0;
    hipLaunchKernelGGL(k_filter_bad_kinect<Ti>, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch(name);
}
extern "C" int kfx_filter_bad_kinect_f32(const kfx_image* out, const kfx_image* in, kfx_stream stream)
{
    return filter_bad_kinect_launch<float>(out, in, "kfx_filter_bad_kinect_f32", stream);
}
extern "C" int kfx_filter_bad_kinect_u16(const kfx_image* out, const kfx_image* in, kfx_stream stream)
{
    return filter_bad_kinect_launch<unsigned short>(out, in, "kfx_filter_bad_kinect_u16", stream);
}

// ColourVbo(dId, dPd, dIc, KT_cd) (cu_depth_tools.cu:86-119)
extern "C" int kfx_colour_vbo(const kfx_image* id, const kfx_image* vbo, const kfx_image* rgb, const float KT_cd[12], kfx_stream stream)
{
    if (int e = check_image(id, 4, 0, 0, "ColourVbo: output image")) return e;
    if (int e = check_image(vbo, 16, cover_w(id), cover_h(id), "ColourVbo: vbo image")) return e;
    if (int e = check_image(rgb, 3, 0, 0, "ColourVbo: rgb image")) return e;
    if (!KT_cd) return set_error(KFX_E_NULL, "ColourVbo: null transform");
    if (id->w == 0 || id->h == 0) return 0;
    ColourVboParams p;
    p.vbo = (const unsigned char*)vbo->ptr; p.vpitch = vbo->pitch;
    p.rgb = (const unsigned char*)rgb->ptr; p.rpitch = rgb->pitch; p.rw = (int)rgb->w; p.rh = (int)rgb->h;
    p.out = (unsigned char*)id->ptr; p.opitch = id->pitch; p.w = (int)id->w; p.h = (int)id->h;
    for (int i = 0; i < 12; ++i) p.KT.m[i] = KT_cd[i];
    hipLaunchKernelGGL(k_colour_vbo, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_colour_vbo");
}

// BilateralFilter(dOut, dIn, dImg, gs, gr, gc, size) (cu_bilateral.cu:145-155): guide image float or unsigned char
template <typename Tg>
static int guided_launch(const kfx_image* out, const kfx_image* in, const kfx_image* guide, float gs, float gr, float gc, unsigned size,
                         kfx_stream stream)
{
    if (int e = check_image(out, 4, 0, 0, "BilateralFilter(guided): output image")) return e;
    if (int e = check_image(in, 4, cover_w(out), cover_h(out), "BilateralFilter(guided): input image")) return e;
    if (int e = check_image(guide, sizeof(Tg), cover_w(out), cover_h(out), "BilateralFilter(guided): guide image")) return e;
    if (out->w == 0 || out->h == 0) return 0;
    if (size > 64) return set_error(KFX_E_RANGE, "BilateralFilter(guided): window too large");
    GuidedParams g;
    g.b = bil_params(out, in, gs, gr, size, 0.f, 0);
    g.guide = (const unsigned char*)guide->ptr;
    g.gpitch = guide->pitch;
    g.gw = (int)guide->w;
    g.gh = (int)guide->h;
    g.gc = gc;
    hipLaunchKernelGGL(k_bilateral_guided<Tg>, pixel_grid(g.b.w, g.b.h), dim3(256), 0, (hipStream_t)stream, g);
    return check_launch("kfx_bilateral_guided");
}
extern "C" int kfx_bilateral_guided_f32(const kfx_image* out, const kfx_image* in, const kfx_image* guide, float gs, float gr, float gc,
                                        unsigned size, kfx_stream stream)
{
    return guided_launch<float>(out, in, guide, gs, gr, gc, size, stream);
}
extern "C" int kfx_bilateral_guided_u8(const kfx_image* out, const kfx_image* in, const kfx_image* guide, float gs, float gr, float gc,
                                       unsigned size, kfx_stream stream)
{
    return guided_launch<unsigned char>(out, in, guide, gs, gr, gc, size, stream);
}

// DepthToVbo<float>(vbo, depth, K, scale) followed by NormalsFromVbo(nrm, vbo), one launch, identical outputs
// (no reference counterpart: a launch-count optimisation for the frame pre-amble; vbo, nrm and depth of one size)
namespace kfx {
int depth_to_vbo_normals_texels(const kfx_image* vbo, const kfx_image* nrm, const kfx_image* depth, const float K[4], float scale,
                                const kfx_image* texels, kfx_stream stream);
}
extern "C" int kfx_depth_to_vbo_normals_f32(const kfx_image* vbo, const kfx_image* nrm, const kfx_image* depth, const float K[4], float scale,
                                            kfx_stream stream)
{
    return kfx::depth_to_vbo_normals_texels(vbo, nrm, depth, K, scale, nullptr, stream);
}
// ... and, for kfx_frame_step, the packed texel image of the SdfFuse that follows from the same launch (texels: w x h float4, or null)
int kfx::depth_to_vbo_normals_texels(const kfx_image* vbo, const kfx_image* nrm, const kfx_image* depth, const float K[4], float scale,
                                     const kfx_image* texels, kfx_stream stream)
{
    if (int e = check_image(vbo, 16, 0, 0, "DepthToVbo+Normals: vbo image")) return e;
    if (int e = check_image(nrm, 16, 0, 0, "DepthToVbo+Normals: normal image")) return e;
    if (int e = check_image(depth, 4, cover_w(vbo), cover_h(vbo), "DepthToVbo+Normals: depth image")) return e;
    if (!K) return set_error(KFX_E_NULL, "DepthToVbo+Normals: null intrinsics");
    if (vbo->w == 0 || vbo->h == 0) return 0;
    if (nrm->w != vbo->w || nrm->h != vbo->h) return set_error(KFX_E_SHAPE, "DepthToVbo+Normals: vbo and normals differ in size");
    // texels: a buffer of tex_layout(w, h).bytes bytes in that layout (host_args.h), its pitch the layout's
    const TexLayout tl = tex_layout(vbo->w, vbo->h);
    if (texels && (!texels->ptr || texels->w != vbo->w || texels->h != vbo->h || texels->pitch != tl.tpitch || ((uintptr_t)texels->ptr & 15)))
        return set_error(KFX_E_SHAPE, "DepthToVbo+Normals: texel image");
    VboNrmParams p{(const unsigned char*)depth->ptr, depth->pitch, (unsigned char*)vbo->ptr, (unsigned char*)nrm->ptr, vbo->pitch, nrm->pitch,
                   (int)vbo->w, (int)vbo->h, Intr{K[0], K[1], K[2], K[3]}, scale, texels ? (unsigned char*)texels->ptr : nullptr, texels ? tl.tpitch : 0,
                   texels ? reinterpret_cast<float*>((unsigned char*)texels->ptr + tl.bmax_off) : nullptr, tl.bw8};
    hipLaunchKernelGGL(k_vbo_normals_f32, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_depth_to_vbo_normals_f32");
}

// ---- the depth pyramid with its vertex and normal maps, one launch (round 5) -------------------------------------------------
// BoxReduceIgnoreInvalid (levels 1 .. L-1 from level 0) followed by DepthToVbo + NormalsFromVbo on every level are 2 L - 1
// launches of 3-5 us each (seven per frame of the tracked loop, profiles/r05_tracked: latency, not work).  Here a workgroup owns
// a 32 x 32 tile of level 0 and the 16 x 16 / 8 x 8 / 4 x 4 tiles below it: it stages the tile with an apron of 8 pixels to the
// right and below in LDS, halves it level by level there (box_half, as k_box_half_ignore_invalid_f32) -- the apron is what the
// next level's one-pixel apron is averaged from, and a level's one-pixel apron holds the neighbours its normals need -- writes
// each level's depth tile, and evaluates depth_vertex / vertex_normal, as k_vbo_normals_f32 does, from the LDS values.  Every
// output is the per-level launches' bit for bit.
struct PyrParams {
    const unsigned char* d0;
    size_t d0_pitch;
    unsigned char* d[4];      // depth of levels 1 .. (index 0 unused)
    size_t dpitch[4];
    unsigned char *vbo[4], *nrm[4];
    size_t vpitch[4], npitch[4];
    int w[4], h[4];
    Intr K[4];
    int levels;
    float scale;
};
__global__ __launch_bounds__(256) void k_depth_pyramid_vbo_normals(const PyrParams p)
{
    constexpr int E0 = 40, E1 = 20, E2 = 10, E3 = 5;   // staged extents: tile + apron
    __shared__ float s0[E0 * E0], s1[E1 * E1], s2[E2 * E2], s3[E3 * E3];
    const int tid = threadIdx.x;
    {   // level 0: the tile and its apron (zero beyond the image: such pixels only feed values nobody reads)
        const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
        for (int t = tid; t < E0 * E0; t += 256) {
            const int ly = t / E0, lx = t - ly * E0, x = x0 + lx, y = y0 + ly;
            s0[t] = (x < p.w[0] && y < p.h[0]) ? reinterpret_cast<const float*>(p.d0 + (size_t)y * p.d0_pitch)[x] : 0.f;
        }
    }
    __syncthreads();
    float* const sl[4] = {s0, s1, s2, s3};
    const int ext[4] = {E0, E1, E2, E3};
#pragma unroll
    for (int l = 1; l < 4; ++l) {
        if (l < p.levels) {   // (uniform)
            const int E = ext[l], Ef = ext[l - 1], S = 32 >> l;
            const int x0 = blockIdx.x * S, y0 = blockIdx.y * S;
            const float* f = sl[l - 1];
            for (int t = tid; t < E * E; t += 256) {
                const int ly = t / E, lx = t - ly * E;
                const float m = box_half(f[(2 * ly) * Ef + 2 * lx], f[(2 * ly) * Ef + 2 * lx + 1], f[(2 * ly + 1) * Ef + 2 * lx], f[(2 * ly + 1) * Ef + 2 * lx + 1]);
                sl[l][t] = m;
                const int x = x0 + lx, y = y0 + ly;
                if (lx < S && ly < S && x < p.w[l] && y < p.h[l]) reinterpret_cast<float*>(p.d[l] + (size_t)y * p.dpitch[l])[x] = m;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (l >= p.levels) break;   // (uniform)
        const int E = ext[l], S = 32 >> l, w = p.w[l], h = p.h[l];
        const int x0 = blockIdx.x * S, y0 = blockIdx.y * S;
        const float* d = sl[l];
        const Intr K = p.K[l];
        for (int t = tid; t < S * S; t += 256) {
            const int ly = t / S, lx = t - ly * S, u = x0 + lx, v = y0 + ly;
            if (u >= w || v >= h) continue;
            const float4 Vc = depth_vertex(K, p.scale * d[ly * E + lx], u, v);
            reinterpret_cast<float4*>(p.vbo[l] + (size_t)v * p.vpitch[l])[u] = Vc;
            float4 N = make_float4(0.f, 0.f, 0.f, 0.f);
            if (u + 1 < w && v + 1 < h)
                N = vertex_normal(Vc, depth_vertex(K, p.scale * d[ly * E + lx + 1], u + 1, v), depth_vertex(K, p.scale * d[(ly + 1) * E + lx], u, v + 1));
            reinterpret_cast<float4*>(p.nrm[l] + (size_t)v * p.npitch[l])[u] = N;
        }
    }
}

// depth[0 .. levels): level 0 is the input, levels 1 .. are written (each at most half the size of the one before, as
// BoxHalfIgnoreInvalid requires); vbo[l] / nrm[l]: the maps of level l, of depth[l]'s size; K: levels x {fu, fv, u0, v0}
extern "C" int kfx_depth_pyramid_vbo_normals_f32(const kfx_image* depth, const kfx_image* vbo, const kfx_image* nrm, const float* K, int levels,
                                                 float scale, kfx_stream stream)
{
    if (!depth || !vbo || !nrm || !K) return set_error(KFX_E_NULL, "DepthPyramidVboNormals: null argument");
    if (levels < 1 || levels > 4) return set_error(KFX_E_RANGE, "DepthPyramidVboNormals: 1 to 4 levels");
    PyrParams p;
    p.levels = levels;
    p.scale = scale;
    for (int l = 0; l < 4; ++l) {
        p.d[l] = p.vbo[l] = p.nrm[l] = nullptr;
        p.dpitch[l] = p.vpitch[l] = p.npitch[l] = 0;
        p.w[l] = p.h[l] = 0;
        p.K[l] = Intr{1.f, 1.f, 0.f, 0.f};
    }
    for (int l = 0; l < levels; ++l) {
        if (int e = check_image(&depth[l], 4, 0, 0, "DepthPyramidVboNormals: depth image")) return e;
        if (int e = check_image(&vbo[l], 16, 0, 0, "DepthPyramidVboNormals: vbo image")) return e;
        if (int e = check_image(&nrm[l], 16, 0, 0, "DepthPyramidVboNormals: normal image")) return e;
        if (vbo[l].w != depth[l].w || vbo[l].h != depth[l].h || nrm[l].w != depth[l].w || nrm[l].h != depth[l].h)
            return set_error(KFX_E_SHAPE, "DepthPyramidVboNormals: the maps of a level differ in size from its depth image");
        if (l > 0 && (depth[l - 1].w < 2 * depth[l].w || depth[l - 1].h < 2 * depth[l].h))
            return set_error(KFX_E_SHAPE, "DepthPyramidVboNormals: a level larger than half the one before");
        if (depth[l].w == 0 || depth[l].h == 0) return set_error(KFX_E_SHAPE, "DepthPyramidVboNormals: empty level");
        p.d[l] = (unsigned char*)depth[l].ptr; p.dpitch[l] = depth[l].pitch;
        p.vbo[l] = (unsigned char*)vbo[l].ptr; p.vpitch[l] = vbo[l].pitch;
        p.nrm[l] = (unsigned char*)nrm[l].ptr; p.npitch[l] = nrm[l].pitch;
        p.w[l] = (int)depth[l].w; p.h[l] = (int)depth[l].h;
        p.K[l] = Intr{K[4 * l], K[4 * l + 1], K[4 * l + 2], K[4 * l + 3]};
    }
    p.d0 = (const unsigned char*)depth[0].ptr;
    p.d0_pitch = depth[0].pitch;
    hipLaunchKernelGGL(k_depth_pyramid_vbo_normals, dim3(ceil_div(p.w[0], 32), ceil_div(p.h[0], 32)), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_depth_pyramid_vbo_normals_f32");
}

// TextureDepth<float4,uchar3>(img, kf, depth, norm, T_wd, Kdepth) (single keyframe: n_kf = 1, phong = NULL) and
// TextureDepth<float4,uchar3,10>(img, kfs, depth, norm, phong, T_wd, Kdepth) (cu_depth_tools.cu:123-207)
extern "C" int kfx_texture_depth(const kfx_image* img, const kfx_keyframe* kfs, int n_kf, const kfx_image* depth, const kfx_image* norm,
                                 const kfx_image* phong, const float T_wd[12], const float Kdepth[4], kfx_stream stream)
{
    if (int e = check_image(img, 16, 0, 0, "TextureDepth: output image")) return e;
    if (int e = check_image(depth, 4, cover_w(img), cover_h(img), "TextureDepth: depth image")) return e;
    if (int e = check_image(norm, 16, cover_w(img), cover_h(img), "TextureDepth: normal image")) return e;
    if (!kfs || n_kf < 1 || n_kf > TEX_MAX_KF || !T_wd || !Kdepth) return set_error(KFX_E_NULL, "TextureDepth: keyframes / transforms");
    const bool single = phong == nullptr;
    if (!single) { if (int e = check_image(phong, 4, cover_w(img), cover_h(img), "TextureDepth: phong image")) return e; }
    if (single && n_kf != 1) return set_error(KFX_E_RANGE, "TextureDepth: the single-keyframe form takes exactly one keyframe");
    if (img->w == 0 || img->h == 0) return 0;
    TextureParams p;
    p.out = (unsigned char*)img->ptr; p.opitch = img->pitch;
    p.depth = (const unsigned char*)depth->ptr; p.dpitch = depth->pitch;
    p.norm = (const unsigned char*)norm->ptr; p.npitch = norm->pitch;
    p.phong = single ? nullptr : (const unsigned char*)phong->ptr; p.ppitch = single ? 0 : phong->pitch;
    p.w = (int)img->w; p.h = (int)img->h; p.nkf = n_kf; p.single = single ? 1 : 0;
    for (int i = 0; i < 12; ++i) p.T_wd.m[i] = T_wd[i];
    p.Kd = Intr{Kdepth[0], Kdepth[1], Kdepth[2], Kdepth[3]};
    for (int k = 0; k < TEX_MAX_KF; ++k) {
        KeyframeView& kv = p.kf[k];
        kv.img = nullptr; kv.pitch = 0; kv.w = kv.h = 0;
        kv.K = Intr{1.f, 1.f, 0.f, 0.f};
        for (int i = 0; i < 12; ++i) kv.T_iw.m[i] = 0.f;
        if (k < n_kf && kfs[k].img.ptr) {
            if (kfs[k].img.pitch < kfs[k].img.w * 3) return set_error(KFX_E_SHAPE, "TextureDepth: keyframe image pitch");
            kv.img = (const unsigned char*)kfs[k].img.ptr; kv.pitch = kfs[k].img.pitch; kv.w = (int)kfs[k].img.w; kv.h = (int)kfs[k].img.h;
            kv.K = Intr{kfs[k].K[0], kfs[k].K[1], kfs[k].K[2], kfs[k].K[3]};
            for (int i = 0; i < 12; ++i) kv.T_iw.m[i] = kfs[k].T_iw[i];
        }
    }
    if (single && !p.kf[0].img) return set_error(KFX_E_NULL, "TextureDepth: keyframe image is null");
    hipLaunchKernelGGL(k_texture_depth, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_texture_depth");
}
