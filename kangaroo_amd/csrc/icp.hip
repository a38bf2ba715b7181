// icp.hip -- projective point-to-plane ICP normal equations (roo::PoseRefinementProjectiveIcpPointPlane)
// for gfx950.  SURVEY.md 8(f) row f-2.
//
// Reference behaviour: src/cu_model_refinement.cu:541-608 (per-pixel residual / Jacobian / Tukey weight),
// LeastSquareSum.h:42-86 (per-block tree reduction in shared memory, then thrust::reduce over the blocks),
// Mat.h:353-545 (SymMat / LeastSquaresSystem: JTy[6], JTJ[21] lower triangle row-major, sqErr, obs).
//
// New kernel: a pixel's 29-word system lives in registers, not in a 116-byte LDS slot per thread.  The
// reference's tree (s[t] += s[t+S], S = n/2 .. 1) is reproduced with the same association: the levels
// S >= 64 cross wavefronts through a structure-of-arrays LDS buffer (conflict-free: word k of lane l at
// k*S + l), the levels S < 64 are wave64 lane shifts -- so a block's sum is bit-identical to the
// reference's.  The sum over blocks (thrust::reduce: order unspecified in the reference) is a fixed order
// here: thread t of one 256-thread group adds blocks t, t+256, ... in turn, then the same tree.
#include <string.h>

#include "kfx_device.h"
#include "host_args.h"

namespace kfx {

constexpr int LSS_WORDS = 29; // 6 JTy + 21 JTJ + sqErr + obs

struct Lss {
    float f[28]; // JTy[0..5], JTJ[0..20], sqErr
    unsigned obs;
};

__device__ __forceinline__ void lss_zero(Lss& s)
{
#pragma unroll
    for (int i = 0; i < 28; ++i) s.f[i] = 0.f;
    s.obs = 0u;
}

// s[t] += s[t+S] for S = n/2 .. 1 (LeastSquareSum.h:71-85); the result is valid in thread 0
__device__ __forceinline__ void lss_tree(Lss& s, const int tid, const int n, float* lds)
{
    for (int S = n >> 1; S >= 64; S >>= 1) {
        __syncthreads();
        if (tid >= S && tid < 2 * S) {
#pragma unroll
            for (int k = 0; k < 28; ++k) lds[k * S + (tid - S)] = s.f[k];
            lds[28 * S + (tid - S)] = __uint_as_float(s.obs);
        }
        __syncthreads();
        if (tid < S) {
#pragma unroll
            for (int k = 0; k < 28; ++k) s.f[k] += lds[k * S + tid];
            s.obs += __float_as_uint(lds[28 * S + tid]);
        }
    }
    if (tid < 64) {
        for (int S = (n >> 1) < 32 ? (n >> 1) : 32; S > 0; S >>= 1) {
#pragma unroll
            for (int k = 0; k < 28; ++k) s.f[k] += __shfl_down(s.f[k], S, 64);
            s.obs += (unsigned)__shfl_down((int)s.obs, S, 64);
        }
    }
}

__device__ __forceinline__ void lss_store(float* dst, const Lss& s)
{
#pragma unroll
    for (int k = 0; k < 28; ++k) dst[k] = s.f[k];
    dst[28] = __uint_as_float(s.obs);
}

// A block system for other workgroups of the same launch to read: device-scope atomic stores go to the device's coherence point,
// past the XCD's L2 (the eight L2s are not coherent with each other); they have arrived when the wave's memory counter has drained.
__device__ __forceinline__ void lss_store_agent(float* dst, const Lss& s)
{
#pragma unroll
    for (int k = 0; k < 28; ++k) __hip_atomic_store(dst + k, s.f[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(dst + 28, __uint_as_float(s.obs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The sum over the blocks' systems in the fixed order: thread t of the 256 adds blocks t, t + 256, ... in turn (lss_tree over the
// 256 partial sums follows).  AgentLoads: the systems were written by other workgroups of this same launch (lss_store_agent), so
// they are read with device-scope atomic loads, which go past this XCD's L2 as the stores did.
template <bool AgentLoads>
__device__ __forceinline__ void lss_block_sum(Lss& acc, const float* sums, const int nblocks, const int tid)
{
    lss_zero(acc);
    for (int b = tid; b < nblocks; b += 256) {
        const float* s = sums + (size_t)b * LSS_WORDS;
        const auto word = [s](const int k) { return AgentLoads ? __hip_atomic_load(s + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : s[k]; };
#pragma unroll
        for (int k = 0; k < 28; ++k) acc.f[k] += word(k);
        acc.obs += __float_as_uint(word(28));
    }
}

// The result mailbox (ResultPort below), 128 bytes of mapped host memory: a kernel writes its payload -- the 29 words of a summed
// system, or the 15 doubles {T, rmse, obs, good} -- and then, system-scope release, the call's sequence number into byte 124.
constexpr int MAILBOX_BYTES = 128, MAILBOX_SEQ_WORD = 31;
__device__ __forceinline__ void mailbox_post(void* mailbox, const unsigned seq)
{
    __hip_atomic_store(reinterpret_cast<unsigned*>(mailbox) + MAILBOX_SEQ_WORD, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct IcpParams {
    ImgView Pl, Pr, Nr;
    unsigned char* dbg; // may be null
    size_t dbg_pitch;
    Pose KT_lr, T_rl;
    const float* dev_pose; // device-resident loop: KT_lr[12] then T_rl[12] live here instead (may be null)
    float c;
    float* sums;        // gridDim.x * gridDim.y systems of 29 words
};

// one pixel's contribution (cu_model_refinement.cu:541-590) and its debug colour
__device__ __forceinline__ void icp_pixel(Lss& sum, float4& dbg, const ImgView& Pl_img, const ImgView& Pr_img, const ImgView& Nr_img, const Pose& KT_lr,
                                          const Pose& T_rl, const float c, const unsigned u, const unsigned v)
{
    const float4 Pr = row<float4>(Pr_img, v)[u];
    const float4 Nr = row<float4>(Nr_img, v)[u];
    const V3 KPl = se3_mul(KT_lr, v3(Pr.x, Pr.y, Pr.z));
    const float plx = KPl.x / KPl.z, ply = KPl.y / KPl.z;
    // Image::InBounds(pl, 3): border <= x && x < (w - border) with w converted to float (Image.h:288-291)
    if (isfinite(Pr.z) && Nr.w == 1.0f && 3.0f <= plx && plx < ((float)Pl_img.w - 3.0f) && 3.0f <= ply && ply < ((float)Pl_img.h - 3.0f)) {
        // GetNearestNeighbour: Get(u + 0.5, v + 0.5) -- the sum is a double, truncated to int (Image.h:337-340)
        const int nx = (int)((double)plx + 0.5), ny = (int)((double)ply + 0.5);
        const float4 Pl = row<float4>(Pl_img, ny)[nx];
        if (isfinite(Pl.z)) {
            const V3 _Pr = se3_mul(T_rl, v3(Pl.x, Pl.y, Pl.z));
            const V3 Dr = v3(_Pr.x - Pr.x, _Pr.y - Pr.y, _Pr.z - Pr.z);
            const V3 N = v3(Nr.x, Nr.y, Nr.z);
            const float y = dot(Dr, N);
            // -dot(SE3gen_i * _Pr, Nr): the generators' zero / one entries are multiplied out as the reference does
            float J[6];
            J[0] = -dot(v3(1.f, 0.f, 0.f), N);
            J[1] = -dot(v3(0.f, 1.f, 0.f), N);
            J[2] = -dot(v3(0.f, 0.f, 1.f), N);
            J[3] = -dot(v3(0.f, -_Pr.z, _Pr.y), N);
            J[4] = -dot(v3(_Pr.z, 0.f, -_Pr.x), N);
            J[5] = -dot(v3(-_Pr.y, _Pr.x, 0.f), N);
            // LSReweightTukey (reweighting.h:22-28)
            const float absr = fabsf(y);
            const float roc = y / c;
            const float omroc2 = 1.0f - roc * roc;
            const float tukey = (absr <= c) ? omroc2 * omroc2 : 0.0f;
            const float w = (1.0f / Pr.z) * tukey;
            const float yw = y * w;
#pragma unroll
            for (int r = 0; r < 6; ++r) sum.f[r] = J[r] * yw;           // mul_aTb(Jr, y*w)
            int i = 6;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int cc = 0; cc <= r; ++cc) sum.f[i++] = J[r] * J[cc] * w; // OuterProduct(Jr, w)
            sum.f[27] = y * y;
            sum.obs = 1u;
            dbg = make_float4(absr, absr, absr, 1.f);
        } else {
            dbg = make_float4(0.f, 0.f, 1.f, 1.f);
        }
    } else {
        dbg = make_float4(1.f, 0.f, 0.f, 1.f);
    }
}

__global__ __launch_bounds__(256) void k_icp_point_plane(const IcpParams p)
{
    extern __shared__ float lds[];
    const int n = blockDim.x * blockDim.y;
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    const unsigned u = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned v = blockIdx.y * blockDim.y + threadIdx.y;

    Lss sum;
    lss_zero(sum);

    Pose KT_lr = p.KT_lr, T_rl = p.T_rl;
    if (p.dev_pose) { // uniform loads: the pose was written by k_lss_final_solve of the previous iteration
#pragma unroll
        for (int i = 0; i < 12; ++i) { KT_lr.m[i] = p.dev_pose[i]; T_rl.m[i] = p.dev_pose[12 + i]; }
    }
    float4 dbg;
    icp_pixel(sum, dbg, p.Pl, p.Pr, p.Nr, KT_lr, T_rl, p.c, u, v);
    if (p.dbg) reinterpret_cast<float4*>(p.dbg + (size_t)v * p.dbg_pitch)[u] = dbg;

    lss_tree(sum, tid, n, lds);
    if (tid == 0) lss_store(p.sums + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * LSS_WORDS, sum);
}

// sum of the per-block systems, fixed order; the result replaces sums[0..28].  mailbox (optional): the system again, then the
// sequence word: the host thread spins on it instead of enqueueing a copy and synchronising the stream (kfx_icp_point_plane).
__global__ __launch_bounds__(256) void k_lss_final(float* sums, const int nblocks, float* mailbox, const unsigned seq)
{
    __shared__ float lds[LSS_WORDS * 128];
    const int tid = threadIdx.x;
    Lss acc;
    lss_block_sum<false>(acc, sums, nblocks, tid);
    lss_tree(acc, tid, 256, lds); // its first __syncthreads orders every read above before the store below
    if (tid == 0) {
        lss_store(sums, acc);
        if (mailbox) {
            lss_store(mailbox, acc);
            mailbox_post(mailbox, seq);
        }
    }
}

// ---------------------------------------------------------------------------------------
// Device-resident refinement loop.  The reference application reads every summed system back, solves it with
// Eigen on the host and uploads the new transforms (main.cpp:301-337): six launch + synchronise + read-back round
// trips per frame.  Here the 6x6 step runs on the GPU as well -- one thread, float64, the same algorithm as
// kangaroo_amd/tracking.py / apps/pose_solve.h (weak prior, rotation-only solve on the coarsest level, LU with
// complete pivoting and Eigen's rank threshold, closed-form SE(3) exponential) -- and leaves K*T_lp / T_lp^-1 in
// device memory for the next k_icp_point_plane.  The host enqueues all iterations back to back and synchronises once.
// State (doubles): T_lp row-major 3x4 [0..11], rmse [12], obs [13], tracking flag [14]; floats: KT_lr[12], T_rl[12].
// ---------------------------------------------------------------------------------------
struct Verdict { double rmse, obs, good; };
struct RefineState {
    double T[12];
    Verdict v;
    float pose[24];
};

// The working set of the solve lives in LDS: the pivoting indexes it with run-time indices, which as per-thread arrays meant
// scratch memory -- 320 scratch instructions in the one-lane solve, each a dependent round trip to memory: 12.5 us per
// k_lss_final_solve, more than the k_icp_point_plane before it (profiles/r05_tracked).  Same arithmetic in the same order.
struct SolveLds {
    double lu[6][6];
    double b[6], c[6], y[6], x[6];
    int rows[6], cols[6];
};

template <int N>
__device__ void lu_solve_full_piv(SolveLds& w, const double* A, const double* b, double* x)
{
    double (&lu)[6][6] = w.lu;
    int (&rows)[6] = w.rows, (&cols)[6] = w.cols;
    for (int i = 0; i < N; ++i) {
        rows[i] = cols[i] = i;
        w.b[i] = b[i];
        for (int j = 0; j < N; ++j) lu[i][j] = A[i * N + j];
    }
    int nonzero = N;
    double maxpivot = 0.0;
    for (int k = 0; k < N; ++k) {
        int pr = k, pc = k;
        double biggest = 0.0;
        for (int i = k; i < N; ++i)
            for (int j = k; j < N; ++j)
                if (fabs(lu[i][j]) > biggest) { biggest = fabs(lu[i][j]); pr = i; pc = j; }
        if (biggest == 0.0) { nonzero = k; break; }
        if (biggest > maxpivot) maxpivot = biggest;
        if (pr != k) {
            for (int j = 0; j < N; ++j) { const double t = lu[k][j]; lu[k][j] = lu[pr][j]; lu[pr][j] = t; }
            const int t = rows[k]; rows[k] = rows[pr]; rows[pr] = t;
        }
        if (pc != k) {
            for (int i = 0; i < N; ++i) { const double t = lu[i][k]; lu[i][k] = lu[i][pc]; lu[i][pc] = t; }
            const int t = cols[k]; cols[k] = cols[pc]; cols[pc] = t;
        }
        const double pivot = lu[k][k];
        for (int i = k + 1; i < N; ++i) {
            const double f = lu[i][k] / pivot;
            lu[i][k] = f;
            for (int j = k + 1; j < N; ++j) lu[i][j] -= f * lu[k][j];
        }
    }
    const double thresh = 2.220446049250313e-16 * N * maxpivot;
    int rank = 0;
    for (int i = 0; i < nonzero; ++i) rank += fabs(lu[i][i]) > thresh ? 1 : 0;
    for (int i = 0; i < N; ++i) w.x[i] = 0.0;
    if (rank != 0) {
        for (int i = 0; i < N; ++i) {
            double ci = w.b[rows[i]];
            for (int j = 0; j < i; ++j) ci -= lu[i][j] * w.c[j];
            w.c[i] = ci;
            w.y[i] = 0.0;
        }
        for (int i = rank - 1; i >= 0; --i) {
            double sum = w.c[i];
            for (int j = i + 1; j < rank; ++j) sum -= lu[i][j] * w.y[j];
            w.y[i] = sum / lu[i][i];
        }
        for (int i = 0; i < N; ++i) w.x[cols[i]] = w.y[i];
    }
    for (int i = 0; i < N; ++i) x[i] = w.x[i];
}

// T <- T * exp(x); rotation_only uses exp(omega) with zero translation
__device__ void se3_right_multiply_exp(double T[12], const double x[6], bool rotation_only)
{
    const double* w = x + 3;
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], t = sqrt(t2);
    const double W[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    double W2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[i][j] = W[i][0] * W[0][j] + W[i][1] * W[1][j] + W[i][2] * W[2][j];
    const bool small = t < 1e-10;
    double st, ct;
    sincos(t, &st, &ct);   // (one argument reduction for both: the values of sin(t) and cos(t))
    const double a = small ? 1.0 : st / t, b = small ? 0.5 : (1.0 - ct) / t2, c = small ? 1.0 / 6.0 : (t - st) / (t2 * t);
    double E[12];
    for (int i = 0; i < 3; ++i) {
        double p = 0.0;
        for (int j = 0; j < 3; ++j) {
            E[i * 4 + j] = (i == j ? 1.0 : 0.0) + a * W[i][j] + b * W2[i][j];
            p += ((i == j ? 1.0 : 0.0) + b * W[i][j] + c * W2[i][j]) * x[j];
        }
        E[i * 4 + 3] = rotation_only ? 0.0 : p;
    }
    double R[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[i * 4 + j] = T[i * 4 + 0] * E[0 * 4 + j] + T[i * 4 + 1] * E[1 * 4 + j] + T[i * 4 + 2] * E[2 * 4 + j];
        R[i * 4 + 3] = T[i * 4 + 0] * E[3] + T[i * 4 + 1] * E[7] + T[i * 4 + 2] * E[11] + T[i * 4 + 3];
    }
    for (int i = 0; i < 12; ++i) T[i] = R[i];
}

// KT_lr = K * T (3x4) and T_rl = T^-1 as floats (host and device: the first evaluation's come from the host, see kfx_icp_refine)
__host__ __device__ inline void pose_floats(float* pose, const float K[4], const double* T)
{
    for (int c = 0; c < 4; ++c) {
        pose[0 * 4 + c] = (float)((double)K[0] * T[0 * 4 + c] + (double)K[2] * T[2 * 4 + c]);
        pose[1 * 4 + c] = (float)((double)K[1] * T[1 * 4 + c] + (double)K[3] * T[2 * 4 + c]);
        pose[2 * 4 + c] = (float)T[2 * 4 + c];
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) pose[12 + i * 4 + j] = (float)T[j * 4 + i];
        pose[12 + i * 4 + 3] = (float)(-(T[0 * 4 + i] * T[3] + T[1 * 4 + i] * T[7] + T[2 * 4 + i] * T[11]));
    }
}
__device__ void publish_pose(RefineState* st, const float K[4], const double* T) { pose_floats(st->pose, K, T); }

__device__ void publish_pose(RefineState* st, const float K[4]) { publish_pose(st, K, st->T); }

struct K4 { float k[4]; };

// element i of the identity pose (row-major 3x4)
__host__ __device__ constexpr double identity12(const int i) { return i % 5 == 0 ? 1.0 : 0.0; }

// the state before any evaluation: the identity, no residual, tracking good; K: intrinsics of the first evaluation's level
__device__ void refine_state_init(RefineState* st, const float K[4])
{
    for (int i = 0; i < 12; ++i) st->T[i] = identity12(i);
    st->v = Verdict{0.0, 0.0, 1.0};
    publish_pose(st, K);
}

__global__ void k_icp_refine_init(RefineState* st, const K4 K) { refine_state_init(st, K.k); }

// what a summed system says about the pose it was evaluated at (main.cpp:334-337)
__device__ __forceinline__ Verdict lss_verdict(const float* sums, const float max_rmse)
{
    const float sq = sums[27];
    const unsigned obs = __float_as_uint(sums[28]);
    const float rmse = sqrtf(sq / (float)obs);
    return Verdict{(double)rmse, (double)obs, rmse < max_rmse ? 1.0 : 0.0};
}

// T <- T * exp(-x_raw), x_raw the solution of the 6 x 6 system (rotation only: of its 3 x 3 block, the translation stays zero).
// A full step with a non-finite component is refused: T is left alone and the result is false.
__device__ bool apply_step(double T[12], const double* x_raw, const bool rotation_only)
{
    double x[6] = {0, 0, 0, 0, 0, 0};
    bool moved = true;
    if (rotation_only) {   // (the flag a literal at either call: one copy of the exponential that takes it at run time cost the chain 1 us per frame, profiles/icp_refactor)
        for (int a = 0; a < 3; ++a) x[3 + a] = -x_raw[a];
        se3_right_multiply_exp(T, x, true);
    } else {
        for (int a = 0; a < 6; ++a) { x[a] = -x_raw[a]; moved = moved && isfinite(x[a]); }
        if (moved) se3_right_multiply_exp(T, x, false);
    }
    return moved;
}

// one Gauss-Newton step from the summed system in sums[0..28] (main.cpp:312-333); K_next: intrinsics of the level the
// NEXT evaluation runs on
__device__ void icp_solve_step(RefineState* st, const float* sums, const int rotation_only, const float max_rmse, const float K_next[4], SolveLds& w)
{
    double JTJ[36], JTy[6], x[6];
    int i = 6;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) {
            const double e = (double)sums[i++];
            JTJ[r * 6 + c] = e;
            JTJ[c * 6 + r] = e;
        }
    for (int r = 0; r < 6; ++r) { JTy[r] = (double)sums[r]; JTJ[r * 7] += 0.1 / 0.2; } // weak pose prior: depthSigma / motionSigma
    st->v = lss_verdict(sums, max_rmse);
    if (rotation_only) {
        double A3[9], b3[3];
        for (int a = 0; a < 3; ++a) {
            b3[a] = JTy[3 + a];
            for (int b = 0; b < 3; ++b) A3[a * 3 + b] = JTJ[(3 + a) * 6 + 3 + b];
        }
        lu_solve_full_piv<3>(w, A3, b3, x);
    } else {
        lu_solve_full_piv<6>(w, JTJ, JTy, x);
    }
    apply_step(st->T, x, rotation_only != 0);
    publish_pose(st, K_next);
}


// ---------------------------------------------------------------------------------------
// The solve by one WAVE instead of one lane (round 5).  A lone lane runs ~3800 dependent instructions (13 us per launch, six
// launches per frame: more than the k_icp_point_plane launches they follow, profiles/r05_tracked); most of them are the
// full-pivot LU -- a 91-element pivot search, swaps and 55 multiply-subtracts, one after the other.  Here lane i * N + j holds
// lu[i][j]: the pivot is a six-step arg-max over the wave (largest magnitude, ties to the first element in row-major order:
// what the serial scan's strict `>` selects) through DPP and lane swaps, the two swaps and the elimination's operands are one round
// of lane gathers, an elimination step is one division and one multiply-subtract in every lane, the substitutions read rows
// and columns through v_readlane.  Every element sees
// the operations of lu_solve_full_piv in the same order with the same operands, so the solution is the serial one bit for bit
// (the persistent launch keeps the one-lane solve: test_gpu_persistent_icp_kernel_equals_the_chain_of_launches
// compares the two).  All 64 lanes of the wave must be active.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double shfl_f64(double v, int src) { return __shfl(v, src, 64); }
__device__ __forceinline__ double readlane_f64(double v, int src)   // src uniform: two v_readlane_b32 instead of the LDS crossbar
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// the pivot candidate of a lane and the better of two: larger magnitude, ties to the smaller lane (= the earlier element in
// row-major order, which is what the serial scan's strict `>` keeps)
struct Pivot { double v; int idx; };
__device__ __forceinline__ Pivot better(const Pivot a, const Pivot b)
{
    const bool take = b.v > a.v || (b.v == a.v && b.idx < a.idx);
    return take ? b : a;
}
template <int CTRL>
__device__ __forceinline__ Pivot pivot_dpp(const Pivot p)   // the candidate of the lane a DPP pattern pairs this one with
{
    Pivot o;
    o.v = __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(p.v), CTRL, 0xF, 0xF, true),
                           __builtin_amdgcn_update_dpp(0, __double2loint(p.v), CTRL, 0xF, 0xF, true));
    o.idx = __builtin_amdgcn_update_dpp(0, p.idx, CTRL, 0xF, 0xF, true);
    return o;
}
// the best candidate of the wave in every lane, without the LDS crossbar: quad permutes, the mirrors of 8 and 16 lanes, then
// v_permlane16_swap / v_permlane32_swap (gfx950), which with both operands equal return the values of both partners
__device__ __forceinline__ Pivot pivot_wave_best(Pivot p)
{
    p = better(p, pivot_dpp<0xB1>(p));    // quad_perm [1,0,3,2]
    p = better(p, pivot_dpp<0x4E>(p));    // quad_perm [2,3,0,1]
    p = better(p, pivot_dpp<0x141>(p));   // row_half_mirror
    p = better(p, pivot_dpp<0x140>(p));   // row_mirror
    {
        const auto h = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(p.v), (unsigned)__double2hiint(p.v), false, false);
        const auto l = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(p.v), (unsigned)__double2loint(p.v), false, false);
        const auto x = __builtin_amdgcn_permlane16_swap((unsigned)p.idx, (unsigned)p.idx, false, false);
        p = better(Pivot{__hiloint2double((int)h[0], (int)l[0]), (int)x[0]}, Pivot{__hiloint2double((int)h[1], (int)l[1]), (int)x[1]});
    }
    {
        const auto h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(p.v), (unsigned)__double2hiint(p.v), false, false);
        const auto l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(p.v), (unsigned)__double2loint(p.v), false, false);
        const auto x = __builtin_amdgcn_permlane32_swap((unsigned)p.idx, (unsigned)p.idx, false, false);
        p = better(Pivot{__hiloint2double((int)h[0], (int)l[0]), (int)x[0]}, Pivot{__hiloint2double((int)h[1], (int)l[1]), (int)x[1]});
    }
    return p;
}

template <int N>
__device__ void lu_solve_wave(const float* sums, SolveLds& w)   // leaves x[0 .. N) in w.x
{
    constexpr int O = 6 - N;   // N = 3 (rotation only): the lower-right block of the system and its last three right-hand sides
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));   // (the lane within the wave, whatever the block's shape)
    const bool in = lane < N * N;
    const int i = in ? lane / N : 0, j = in ? lane % N : 0;
    double a = 0.0;
    {
        const int r = O + i, c = O + j, hi = r > c ? r : c, lo = r > c ? c : r;
        const double e = (double)sums[6 + hi * (hi + 1) / 2 + lo];
        a = i == j ? e + 0.1 / 0.2 : e;   // weak pose prior on the diagonal: depthSigma / motionSigma
        if (!in) a = 0.0;
    }
    int rl = lane, cl = lane;   // rows[lane], cols[lane] (lanes below N)
    int nonzero = N;
    double maxpivot = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const Pivot best = pivot_wave_best(Pivot{(in && i >= k && j >= k && fabs(a) > 0.0) ? fabs(a) : -1.0, lane});
        if (!(best.v > 0.0)) { nonzero = k; break; }   // (uniform: every lane holds the same candidate)
        if (best.v > maxpivot) maxpivot = best.v;
        const int idx = __builtin_amdgcn_readfirstlane(best.idx);
        const int pr = idx / N, pc = idx % N;
        // rows k and pr, then columns k and pc change places: element (i, j) comes from (si, sj), its column-k and row-k
        // partners of the elimination from (si, pc) and (pr, sj), the pivot from (pr, pc) -- one round of gathers
        const int si = i == k ? pr : (i == pr ? k : i), sj = j == k ? pc : (j == pc ? k : j);
        const double pivot = readlane_f64(a, idx);
        const double aij = shfl_f64(a, in ? si * N + sj : lane), aik = shfl_f64(a, in ? si * N + pc : lane), akj = shfl_f64(a, in ? pr * N + sj : lane);
        rl = __shfl(rl, lane == k ? pr : (lane == pr ? k : lane), 64);
        cl = __shfl(cl, lane == k ? pc : (lane == pc ? k : lane), 64);
        const double f = aik / pivot;
        a = aij;
        if (in && i > k) {
            if (j == k) a = f;
            else if (j > k) a = aij - f * akj;
        }
    }
    const double thresh = 2.220446049250313e-16 * N * maxpivot;
    const int rank = __popcll(__ballot(in && i == j && i < nonzero && fabs(a) > thresh));
    if (lane < N) w.x[lane] = 0.0;
    if (rank == 0) return;   // (uniform)
    // c[i] = b[rows[i]] - sum_{j < i} lu[i][j] c[j], j ascending
    const double bl = lane < N ? (double)sums[O + lane] : 0.0;
    double c = shfl_f64(bl, lane < N ? rl : lane);
#pragma unroll
    for (int jj = 0; jj < N - 1; ++jj) {
        const double cj = readlane_f64(c, jj), lij = shfl_f64(a, lane < N ? lane * N + jj : lane);
        if (lane < N && lane > jj) c = c - lij * cj;
    }
    // y[i] = (c[i] - sum_{i < j < rank} lu[i][j] y[j]) / lu[i][i], i descending, j ascending (every lane follows the same chain)
    double y = 0.0;
    for (int ii = rank - 1; ii >= 0; --ii) {
        double sum = readlane_f64(c, ii);
        for (int jj = ii + 1; jj < rank; ++jj) sum = sum - readlane_f64(a, ii * N + jj) * readlane_f64(y, jj);
        const double yi = sum / readlane_f64(a, ii * N + ii);
        if (lane == ii) y = yi;
    }
    if (lane < N) w.x[cl] = y;   // x[cols[i]] = y[i]: cols is a permutation
}

// icp_solve_step with the LU spread over the calling wave (all 64 lanes active); lane 0 does what remains
// T_lane: st->T[lane] in lanes 0 .. 11, requested by the caller before the block sums were added up (one memory round trip
// less on the one-lane tail)
// always_store: write T even when the step is refused (the first evaluation of a call: st->T still holds the previous call's pose)
// mailbox (optional): the call's result {T, rmse, obs, good} goes there too, then the sequence word the host spins on
// (kfx_icp_refine: no copy command for the read-back)
__device__ void icp_solve_step_wave(RefineState* st, const float* sums, const int rotation_only, const float max_rmse, const float K_next[4], SolveLds& w,
                                    const double T_lane, const bool always_store = false, double* mailbox = nullptr, const unsigned seq = 0u)
{
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));   // (the lane within the wave, whatever the block's shape)
    if (rotation_only) lu_solve_wave<3>(sums, w);
    else lu_solve_wave<6>(sums, w);
    __builtin_amdgcn_wave_barrier();   // (one wave: its LDS operations complete in order)
    double T[12];
#pragma unroll
    for (int m = 0; m < 12; ++m) T[m] = readlane_f64(T_lane, m);
    if (lane != 0) return;
    const Verdict v = st->v = lss_verdict(sums, max_rmse);
    const bool moved = apply_step(T, w.x, rotation_only != 0);
    if (moved || always_store)
        for (int m = 0; m < 12; ++m) st->T[m] = T[m];
    publish_pose(st, K_next, T);
    if (mailbox) {   // (T is what st->T holds now: the step, or the pose before it when the step was refused)
        for (int m = 0; m < 12; ++m) mailbox[m] = T[m];
        mailbox[12] = v.rmse; mailbox[13] = v.obs; mailbox[14] = v.good;
        mailbox_post(mailbox, seq);
    }
}

// k_lss_final followed by the 6x6 step as one launch (the device-resident loop is a chain of ~5 us kernels: every launch saved is
// time saved).  Thread 0 holds the summed system after the tree; it stores it (so sums[0..28] is what k_lss_final leaves) and
// the first wave solves it.
// first: the first evaluation of a kfx_icp_refine call -- the pose before the step is the identity (no initialising launch)
__global__ __launch_bounds__(256) void k_lss_final_solve(float* sums, const int nblocks, RefineState* st, const int rotation_only,
                                                         const float max_rmse, const K4 K_next, const int first, double* mailbox, const unsigned seq)
{
    __shared__ float lds[LSS_WORDS * 128];
    __shared__ float s_sum[LSS_WORDS];
    __shared__ SolveLds s_solve;
    const int tid = threadIdx.x;
    const double T_lane = tid < 12 ? (first ? identity12(tid) : st->T[tid]) : 0.0;   // (for the tail of the solve: on its way while the sums are added up)
    Lss acc;
    lss_block_sum<false>(acc, sums, nblocks, tid);
    lss_tree(acc, tid, 256, lds);
    if (tid == 0) {
        lss_store(sums, acc);
        lss_store(s_sum, acc);
    }
    __syncthreads();
    if (tid < 64) icp_solve_step_wave(st, s_sum, rotation_only, max_rmse, K_next.k, s_solve, T_lane, first != 0, mailbox, seq);
}

// ---------------------------------------------------------------------------------------
// The whole refinement -- every level, every iteration -- as ONE launch (round-4 verdict, item 6: the chain above was 13 launches
// of 5-9 us of work each, and a frame's budget is 0.4 ms).  A fixed number of workgroups stays resident and walks the schedule:
//   A. the workgroups share out the level's pixel blocks (the reference's launch geometry: gcd(w, 16) x gcd(h, 16) pixels,
//      launch_utils.h:61-65) and leave each block's system in `sums` -- the same per-pixel function, the same tree
//      (lss_tree), so the same bits as k_icp_point_plane;
//   B. one grid-wide barrier (an arrival counter and a generation word in device memory: release fence + atomic add; the last
//      one to arrive advances the generation, the others poll it with s_sleep between two looks, then an acquire fence);
//   C. EVERY workgroup adds up the blocks' systems in k_lss_final's fixed order and takes the 6 x 6 step by itself (thread 0,
//      float64: deterministic, so all workgroups hold the same pose without a second barrier or a broadcast); workgroup 0 leaves
//      the result in the RefineState.
// `sums` is double-buffered by iteration parity: a workgroup may already be writing the next iteration's block systems while a
// slower one still adds up this iteration's.  Every poll is bounded: if a workgroup never arrives (the grid was not resident
// after all), the others set the abort word, leave, and the host reports KFX_E_RANGE instead of waiting for a watchdog.
// The grid is at most the device's resident capacity for this kernel (hipOccupancyMaxActiveBlocksPerMultiprocessor).
// ---------------------------------------------------------------------------------------
struct IcpLevelDev {
    ImgView Pl, Pr, Nr;
    float K[4];
    int iterations, rotation_only;
    int bx, by, gx, gy;   // block shape (pixels), blocks along x / y
};
struct IcpPersistent {
    IcpLevelDev lv[4];
    int n_levels;
    float c, max_rmse;
    unsigned char* dbg;
    size_t dbg_pitch;
    int dbg_w, dbg_h;
    float* sums[2];        // block systems, by iteration parity
    RefineState* st;       // result (workgroup 0)
    unsigned* bar;         // [0] arrivals, [1] generation, [2] abort
};

// The block systems cross workgroups (and XCDs) through device-scope atomic stores and loads (lss_store_agent), so that the barrier
// needs no cache-wide release / acquire (an agent-scope fence writes back and invalidates a whole L2: measured, it made the
// persistent launch slower than the chain of launches).
__device__ __forceinline__ bool grid_barrier(unsigned* bar, const unsigned n_groups, unsigned& gen)
{
    __shared__ int s_ok;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        int ok = 1;
        __builtin_amdgcn_s_waitcnt(0);   // this workgroup's block systems (thread 0 stored them) have reached the coherence point
        const unsigned arrived = __hip_atomic_fetch_add(&bar[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == n_groups - 1) {
            __hip_atomic_store(&bar[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_s_waitcnt(0);
            __hip_atomic_store(&bar[1], gen + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            unsigned spins = 0;
            while (__hip_atomic_load(&bar[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
                if (__hip_atomic_load(&bar[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u || ++spins > (1u << 22)) {   // ~ a second
                    __hip_atomic_store(&bar[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    ok = 0;
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
        }
        s_ok = ok;
    }
    __syncthreads();
    gen += 1;
    return s_ok != 0;
}

// the next level after l that is evaluated, or -1
__device__ __forceinline__ int next_active(const IcpPersistent& q, const int l)
{
    for (int m = l + 1; m < q.n_levels; ++m)
        if (q.lv[m].iterations > 0 && q.lv[m].gx > 0 && q.lv[m].gy > 0) return m;
    return -1;
}

__global__ __launch_bounds__(256) void k_icp_refine_persistent(const IcpPersistent q)
{
    __shared__ float lds[LSS_WORDS * 128];
    __shared__ float s_sum[LSS_WORDS];
    __shared__ SolveLds s_solve;
    __shared__ RefineState s_st;
    const int tid = threadIdx.x;
    const unsigned G = gridDim.x;
    unsigned gen = 0;   // (the host zeroes the barrier words before the launch)
    const int first = next_active(q, -1);
    if (tid == 0) {
        float k0[4] = {0.f, 0.f, 0.f, 0.f};
        if (first >= 0) for (int i = 0; i < 4; ++i) k0[i] = q.lv[first].K[i];
        refine_state_init(&s_st, k0);
    }
    __syncthreads();
    int parity = 0;
    bool alive = true;
    for (int l = 0; l < q.n_levels && alive; ++l) {
        const IcpLevelDev& L = q.lv[l];
        if (L.iterations <= 0 || L.gx <= 0 || L.gy <= 0) continue;
        const int n = L.bx * L.by, nblocks = L.gx * L.gy;
        const int tx = tid % L.bx, ty = tid / L.bx;
        const int nxt = next_active(q, l);
        const bool dbg_on = q.dbg && q.dbg_w >= L.Pl.w && q.dbg_h >= L.Pl.h;
        for (int it = 0; it < L.iterations && alive; ++it, parity ^= 1) {
            float* sums = q.sums[parity];
            Pose KT_lr, T_rl;
#pragma unroll
            for (int i = 0; i < 12; ++i) { KT_lr.m[i] = s_st.pose[i]; T_rl.m[i] = s_st.pose[12 + i]; }
            // ---- A: this workgroup's share of the pixel blocks ----
            for (int b = (int)blockIdx.x; b < nblocks; b += (int)G) {
                const unsigned u = (unsigned)((b % L.gx) * L.bx + tx), v = (unsigned)((b / L.gx) * L.by + ty);
                Lss sum;
                lss_zero(sum);
                if (tid < n) {
                    float4 dbg;
                    icp_pixel(sum, dbg, L.Pl, L.Pr, L.Nr, KT_lr, T_rl, q.c, u, v);
                    if (dbg_on) reinterpret_cast<float4*>(q.dbg + (size_t)v * q.dbg_pitch)[u] = dbg;
                }
                lss_tree(sum, tid, n, lds);
                if (tid == 0) lss_store_agent(sums + (size_t)b * LSS_WORDS, sum);
                __syncthreads();   // (lds is reused by the next block's tree)
            }
            // ---- B ----
            alive = grid_barrier(q.bar, G, gen);
            if (!alive) break;
            // ---- C: the sum over the blocks in k_lss_final's order, and the step ----
            Lss acc;
            lss_block_sum<true>(acc, sums, nblocks, tid);
            lss_tree(acc, tid, 256, lds);
            if (tid == 0) {
                lss_store(s_sum, acc);
                const float* Kn = (it + 1 < L.iterations || nxt < 0) ? L.K : q.lv[nxt].K;
                float kn[4] = {Kn[0], Kn[1], Kn[2], Kn[3]};
                icp_solve_step(&s_st, s_sum, L.rotation_only, q.max_rmse, kn, s_solve);
            }
            __syncthreads();
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (!alive) s_st.v.good = -1.0;   // the grid never met: reported by the host
        *q.st = s_st;
    }
}

static unsigned gcd_u(unsigned a, unsigned b) { return b == 0 ? a : gcd_u(b, a % b); }

// How one level is launched: InitDimFromOutputImage(dPl, 16, 16) (launch_utils.h:61-65) -- blocks of gcd(w, 16) x gcd(h, 16) pixels,
// w / bx x h / by of them (none for an empty image) -- and the LDS of lss_tree's levels that cross wavefronts.  n: pixels
// (= threads) of a block; active: the level is evaluated at all (kfx_icp_point_plane: iterations = 1).
struct IcpGeom { unsigned bx, by, gx, gy; int n; size_t blocks, lds_bytes; bool active; };
static IcpGeom icp_geom(const kfx_image& Pl, int iterations)
{
    IcpGeom g;
    g.bx = gcd_u((unsigned)Pl.w, 16); g.by = gcd_u((unsigned)Pl.h, 16);
    g.gx = (unsigned)(Pl.w / g.bx); g.gy = (unsigned)(Pl.h / g.by);
    g.n = (int)(g.bx * g.by); g.blocks = (size_t)g.gx * g.gy;
    g.lds_bytes = g.n >= 128 ? (size_t)LSS_WORDS * (g.n / 2) * sizeof(float) : 0;
    g.active = iterations > 0 && Pl.w && Pl.h;
    return g;
}
// the next level after l that is evaluated, or -1 (l = -1: the first)
static int next_active(const kfx_icp_level* levels, int n_levels, int l)
{
    for (int m = l + 1; m < n_levels; ++m)
        if (icp_geom(levels[m].Pl, levels[m].iterations).active) return m;
    return -1;
}

// one evaluation's arguments but for the pose; debug: null where the level does not write one
static IcpParams icp_params(const kfx_image& Pl, const kfx_image& Pr, const kfx_image& Nr, const kfx_image* debug, float c, float* sums)
{
    IcpParams p = {};
    p.Pl = img_view(Pl); p.Pr = img_view(Pr); p.Nr = img_view(Nr);
    p.dbg = debug ? (unsigned char*)debug->ptr : nullptr;
    p.dbg_pitch = debug ? debug->pitch : 0;
    p.c = c;
    p.sums = sums;
    return p;
}

// a spinning thread's hint to its core; nothing where the host has none
#if defined(__x86_64__) || defined(__i386__)
#define KFX_SPIN_HINT() __builtin_ia32_pause()
#elif defined(__aarch64__) || defined(__arm__)
#define KFX_SPIN_HINT() __asm__ __volatile__("yield")
#else
#define KFX_SPIN_HINT() ((void)0)
#endif

// A result's way to the host, one per calling thread, shared by kfx_icp_point_plane (the reference's thrust::reduce blocks too; the
// application solves on the host between two of these calls, six times per frame, main.cpp:301-342) and kfx_icp_refine.
//  * The mailbox: 128 bytes of page-locked, portable host memory mapped into the device's address space.  The call's last kernel
//    writes the payload and then the call's sequence number there and this thread spins on that word -- no copy command, no stream
//    synchronisation, no wait for an event (profiles/r06_tracked: the copy's own 4.3 us and the wake-up after hipStreamSynchronize
//    were 8 % of the drop-in application's frame; 4 us of the stream per frame for kfx_icp_refine).
//  * KFX_ICP_MAILBOX=0, no mapped memory, or a word that did not arrive: the round-5 path, a copy into a pinned staging buffer (a
//    device -> pageable copy is staged by the runtime and costs a second synchronisation; without pinned memory it is that copy).
// The hook of kfx_icp_refine_then (enqueue_more: work that does not depend on the result, the next frame's pre-amble) is called
// exactly ONCE per successfully enqueued call: before the spin on the mailbox path -- the copy after a word that did not arrive
// does not call it again -- else between the copy and the wait, which is on an event: for the copy only, not for the hook's work.
struct ResultPort {
    void *mail = nullptr, *mail_dev = nullptr;   // the mailbox's host address, and its device address on device mail_device
    int mail_device = -1;
    unsigned seq = 0;                            // of the last call through the mailbox; never 0, the word's initial value
    void* stage = nullptr;
    hipEvent_t copied = nullptr;
    ~ResultPort()   // rank threads come and go: the pages go back (errors ignored and cleared: the runtime may already be gone)
    {
        if (mail) (void)hipHostFree(mail);
        if (stage) (void)hipHostFree(stage);
        if (copied) (void)hipEventDestroy(copied);
        (void)hipGetLastError();
    }
    // the mailbox's address on the device that is current now (another one than at the last call: asked for again); null: take
    // the copy path (KFX_ICP_MAILBOX=0, or no mapped memory)
    void* mailbox()
    {
        static const bool on = env_int("KFX_ICP_MAILBOX", 1) != 0;
        int dev = 0;
        if (!on || hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (!mail) {
            if (hipHostMalloc(&mail, MAILBOX_BYTES, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); mail = nullptr; return nullptr; }
            memset(mail, 0, MAILBOX_BYTES);
        }
        if (mail_device != dev) {
            if (hipHostGetDevicePointer(&mail_dev, mail, 0) != hipSuccess) { (void)hipGetLastError(); mail_device = -1; return nullptr; }
            mail_device = dev;
        }
        return mail_dev;
    }
    unsigned next_seq() { return ++seq ? seq : ++seq; }
    // Has the word arrived?  Bounded: every 4096 looks the stream is asked whether it is still running -- a launch that failed on the
    // device, or a word that never arrives, ends in the copy path instead of a hang.
    bool wait_mailbox(unsigned want, hipStream_t stream) const
    {
        const unsigned* word = static_cast<const unsigned*>(mail) + MAILBOX_SEQ_WORD;
        for (unsigned spins = 0;; ++spins) {
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return true;
            KFX_SPIN_HINT();
            if ((spins & 4095u) == 4095u && hipStreamQuery(stream) != hipErrorNotReady) {   // finished (or failed): one last look
                (void)hipGetLastError();
                return __atomic_load_n(word, __ATOMIC_ACQUIRE) == want;
            }
        }
    }
    // dst[0 .. bytes) <- device memory at src (bytes <= 128), blocking
    int read_back(void* dst, const void* src, size_t bytes, hipStream_t stream, void (*enqueue_more)(void*), void* user)
    {
        if (!stage && hipHostMalloc(&stage, MAILBOX_BYTES, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); stage = nullptr; }
        void* to = stage ? stage : dst;
        hipError_t e = hipMemcpyAsync(to, src, bytes, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && enqueue_more) {
            if (!copied) e = hipEventCreateWithFlags(&copied, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(copied, stream);
            if (e == hipSuccess) { enqueue_more(user); e = hipEventSynchronize(copied); }
        } else if (e == hipSuccess) {
            e = hipStreamSynchronize(stream);
        }
        if (e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
        if (to != dst) memcpy(dst, to, bytes);
        return 0;
    }
};
static thread_local ResultPort result_port;

// a RefineState's first 15 doubles {T, rmse, obs, good} into the caller's variables
static void deliver(const double r[15], double T_lp[12], float* rmse, unsigned* obs, int* tracking_good)
{
    for (int i = 0; i < 12; ++i) T_lp[i] = r[i];
    if (rmse) *rmse = (float)r[12];
    if (obs) *obs = (unsigned)r[13];
    if (tracking_good) *tracking_good = r[14] != 0.0 ? 1 : 0;
}

} // namespace kfx

using namespace kfx;

// the float4 maps of one level: dPr / dNr cover dPl; a debug image, when given, covers dbg_w x dbg_h
static int check_icp_images(const kfx_image* Pl, const kfx_image* Pr, const kfx_image* Nr, const kfx_image* debug, size_t dbg_w, size_t dbg_h, const char* what)
{
    if (int e = check_image(Pl, 16, 0, 0, what)) return e;
    if (int e = check_image(Pr, 16, Pl->w, Pl->h, what)) return e;
    if (int e = check_image(Nr, 16, Pl->w, Pl->h, what)) return e;
    return debug ? check_image(debug, 16, dbg_w, dbg_h, what) : 0;
}

// LeastSquaresSystem<float,6> PoseRefinementProjectiveIcpPointPlane(dPl, dPr, dNr, KT_lr, T_rl, c, dWorkspace,
// dDebug) (cu_model_refinement.cu:595-608).  Blocks until the 116-byte result is on the host (ResultPort).
extern "C" int kfx_icp_point_plane(const kfx_image* Pl, const kfx_image* Pr, const kfx_image* Nr, const float KT_lr[12],
                                   const float T_rl[12], float c, const kfx_image* workspace, const kfx_image* debug,
                                   kfx_lss6* out, kfx_stream stream)
{
    static_assert(sizeof(kfx_lss6) == LSS_WORDS * 4, "LeastSquaresSystem<float,6> layout");
    if (!Pl || !Pr || !Nr || !KT_lr || !T_rl || !workspace || !out || !Pl->ptr || !Pr->ptr || !Nr->ptr || !workspace->ptr)
        return set_error(KFX_E_NULL, "PoseRefinementProjectiveIcpPointPlane: null argument");
    memset(out, 0, sizeof(*out));
    if (Pl->w == 0 || Pl->h == 0) return 0;
    if (debug && !debug->ptr) debug = nullptr;
    if (int e = check_icp_images(Pl, Pr, Nr, debug, Pl->w, Pl->h, "PoseRefinementProjectiveIcpPointPlane")) return e;
    if ((uintptr_t)workspace->ptr & 3) return set_error(KFX_E_ALIGN, "PoseRefinementProjectiveIcpPointPlane: workspace alignment");
    const IcpGeom g = icp_geom(*Pl, 1);
    // Image::PackedImage asserts the workspace holds gridDim.x * gridDim.y systems (Image.h:464-468)
    if (g.blocks * sizeof(kfx_lss6) > workspace->pitch * workspace->h)
        return set_error(KFX_E_SHAPE, "PoseRefinementProjectiveIcpPointPlane: workspace too small");
    if (g.blocks > 0x7fffffff) return set_error(KFX_E_RANGE, "PoseRefinementProjectiveIcpPointPlane: image too large");
    const hipStream_t s = (hipStream_t)stream;
    IcpParams p = icp_params(*Pl, *Pr, *Nr, debug, c, (float*)workspace->ptr);
    for (int i = 0; i < 12; ++i) { p.KT_lr.m[i] = KT_lr[i]; p.T_rl.m[i] = T_rl[i]; }
    void* mail = result_port.mailbox();
    const unsigned seq = mail ? result_port.next_seq() : 0u;
    hipLaunchKernelGGL(k_icp_point_plane, dim3(g.gx, g.gy), dim3(g.bx, g.by), g.lds_bytes, s, p);
    hipLaunchKernelGGL(k_lss_final, dim3(1), dim3(256), 0, s, p.sums, (int)g.blocks, (float*)mail, seq);
    if (int e = check_launch("kfx_icp_point_plane")) return e;
    if (mail && result_port.wait_mailbox(seq, s)) {
        memcpy(out, result_port.mail, sizeof(*out));
        return 0;
    }
    return result_port.read_back(out, p.sums, sizeof(*out), s, nullptr, nullptr);
}

// The coarse-to-fine loop of main.cpp:301-337 enqueued as one chain of kernels: for every level (coarsest first) and
// iteration, k_icp_point_plane -> k_lss_final_solve (block sum + 6x6 step), all on `stream`, one synchronisation at the end.
// levels[l]: the three vertex / normal maps, the level's intrinsics and its iteration count, given COARSEST FIRST;
// the first level with more than one level in total is solved for rotation only, as the application does.
// workspace: >= max over levels of (blocks * 116) + 512 bytes; result: T_lp (row-major 3x4, float64), rmse, obs,
// tracking_good (rmse < max_rmse at the last evaluation).
static int icp_refine_impl(const kfx_icp_level* levels, int n_levels, float c, float max_rmse, const kfx_image* workspace,
                           const kfx_image* debug, double T_lp[12], float* rmse, unsigned* obs, int* tracking_good, void (*enqueue_more)(void*),
                           void* user, kfx_stream stream)
{
    if (!levels || n_levels <= 0 || !workspace || !workspace->ptr || !T_lp) return set_error(KFX_E_NULL, "kfx_icp_refine: null argument");
    if (debug && !debug->ptr) debug = nullptr;
    size_t max_blocks = 0;
    int evaluations = 0;
    for (int l = 0; l < n_levels; ++l) {
        const kfx_icp_level& L = levels[l];
        // (a debug image smaller than a level is not written at that level)
        if (int e = check_icp_images(&L.Pl, &L.Pr, &L.Nr, debug, 0, 0, "kfx_icp_refine")) return e;
        const IcpGeom g = icp_geom(L.Pl, L.iterations);
        if (g.blocks > max_blocks) max_blocks = g.blocks;
        if (g.active) evaluations += L.iterations;
    }
    const size_t state_off = (max_blocks * sizeof(kfx_lss6) + 255) / 256 * 256;
    if (state_off + sizeof(RefineState) > workspace->pitch * workspace->h || ((uintptr_t)workspace->ptr & 7))
        return set_error(KFX_E_SHAPE, "kfx_icp_refine: workspace too small or misaligned");
    hipStream_t s = (hipStream_t)stream;
    float* sums = (float*)workspace->ptr;
    RefineState* st = (RefineState*)((unsigned char*)workspace->ptr + state_off);
    // KFX_ICP_PERSISTENT=1: one persistent launch (k_icp_refine_persistent) where the workspace has room for the second set of block
    // systems and the barrier words, the levels fit its table (a block's gcd(w, 16) x gcd(h, 16) pixels always fit its 256 threads)
    // and the device can hold the grid.  Same bits as the chain of launches
    // below, which stays the default: measured on MI355X (512^3 tracked frame, C++ loop) the chain takes 0.655 ms per frame, the
    // persistent launch 0.754 (128 workgroups) - 0.844 ms (512) -- a grid-wide barrier across the eight XCDs and a 6 x 6 float64
    // step in every workgroup cost more than the launch boundaries they replace (EXPERIMENTS.md 7.3).
    static const int persistent_env = env_int("KFX_ICP_PERSISTENT", 0);
    const size_t sums2_off = (state_off + sizeof(RefineState) + 255) / 256 * 256, bar_off = sums2_off + state_off;
    // the copy path's end (hook: null where it has been called already)
    const auto copy_result = [&](void (*hook)(void*)) {
        double r[15];
        if (int e = result_port.read_back(r, st, sizeof(r), s, hook, user)) return e;
        if (r[14] < 0.0) return set_error(KFX_E_RANGE, "kfx_icp_refine: the persistent grid never met at its barrier (not resident)");
        deliver(r, T_lp, rmse, obs, tracking_good);
        return 0;
    };
    if (persistent_env != 0 && n_levels <= 4 && bar_off + 256 <= workspace->pitch * workspace->h) {
        static int capacity = -1;   // workgroups of this kernel the device holds at once
        if (capacity < 0) {
            int dev = 0, cus = 0, per_cu = 0;
            if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_icp_refine_persistent, 256, 0) == hipSuccess)
                capacity = cus * (per_cu < 2 ? per_cu : 2);   // two per CU are plenty (a level has at most a few blocks per workgroup); well inside what fits
            else
                capacity = 0;
            (void)hipGetLastError();
        }
        if (capacity >= 1) {
            IcpPersistent q;
            memset(&q, 0, sizeof(q));
            size_t most = 1;
            for (int l = 0; l < n_levels; ++l) {
                const kfx_icp_level& L = levels[l];
                const IcpGeom g = icp_geom(L.Pl, L.iterations);
                IcpLevelDev& d = q.lv[l];
                d.iterations = g.active ? L.iterations : 0;
                d.rotation_only = L.rotation_only ? 1 : 0;
                for (int i = 0; i < 4; ++i) d.K[i] = L.K[i];
                if (!g.active) continue;
                d.Pl = img_view(L.Pl); d.Pr = img_view(L.Pr); d.Nr = img_view(L.Nr);
                d.bx = (int)g.bx; d.by = (int)g.by;
                d.gx = (int)g.gx; d.gy = (int)g.gy;
                if (g.blocks > most) most = g.blocks;
            }
            q.n_levels = n_levels;
            q.c = c; q.max_rmse = max_rmse;
            q.dbg = debug ? (unsigned char*)debug->ptr : nullptr;
            q.dbg_pitch = debug ? debug->pitch : 0;
            q.dbg_w = debug ? (int)debug->w : 0; q.dbg_h = debug ? (int)debug->h : 0;
            q.sums[0] = sums;
            q.sums[1] = (float*)((unsigned char*)workspace->ptr + sums2_off);
            q.st = st;
            q.bar = (unsigned*)((unsigned char*)workspace->ptr + bar_off);
            static const int grid_env = env_int("KFX_ICP_GRID", 0);   // (A/B: cap on the resident workgroups)
            size_t want = (size_t)capacity < most ? (size_t)capacity : most;
            if (grid_env > 0 && (size_t)grid_env < want) want = (size_t)grid_env;
            const unsigned grid = (unsigned)want;
            hipError_t he = hipMemsetAsync(q.bar, 0, 64, s);
            if (he != hipSuccess) { (void)hipGetLastError(); return set_error((int)he, "kfx_icp_refine: hipMemsetAsync"); }
            hipLaunchKernelGGL(k_icp_refine_persistent, dim3(grid), dim3(256), 0, s, q);
            if (int e = check_launch("kfx_icp_refine")) return e;
            return copy_result(enqueue_more);
        }
    }
    // every solve knows the intrinsics of the evaluation that follows it
    const int first = next_active(levels, n_levels, -1);
    K4 k0;
    for (int i = 0; i < 4; ++i) k0.k[i] = first >= 0 ? levels[first].K[i] : 0.f;
    // The pose starts at the identity: the first evaluation takes K * I and I^-1 as launch arguments (the floats pose_floats gives:
    // what the initialising launch used to leave in device memory) and its solve starts from the identity itself -- one launch
    // less per call.  Only a call without any evaluation initialises the state by a launch (it returns the identity).
    float pose0[24];
    const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    pose_floats(pose0, k0.k, I12);
    if (first < 0) hipLaunchKernelGGL(k_icp_refine_init, dim3(1), dim3(1), 0, s, st, k0);
    // the LAST solve leaves {T, rmse, obs, good} in the mailbox as well (a call without any evaluation has no solve: the copy path)
    void* mail = evaluations > 0 ? result_port.mailbox() : nullptr;
    const unsigned seq = mail ? result_port.next_seq() : 0u;
    int evaluation = 0;
    for (int l = 0; l < n_levels; ++l) {
        const kfx_icp_level& L = levels[l];
        const IcpGeom g = icp_geom(L.Pl, L.iterations);
        if (!g.active) continue;
        const bool dbg = debug && debug->w >= L.Pl.w && debug->h >= L.Pl.h;
        IcpParams p = icp_params(L.Pl, L.Pr, L.Nr, dbg ? debug : nullptr, c, sums);
        // next evaluation's intrinsics: this level while iterations remain, else the next level that has any
        const int nxt = next_active(levels, n_levels, l);
        for (int it = 0; it < L.iterations; ++it) {
            K4 kn;
            const float* Kn = (it + 1 < L.iterations || nxt < 0) ? L.K : levels[nxt].K;
            for (int i = 0; i < 4; ++i) kn.k[i] = Kn[i];
            const bool first_eval = evaluation == 0, last = ++evaluation == evaluations;
            if (first_eval) for (int i = 0; i < 12; ++i) { p.KT_lr.m[i] = pose0[i]; p.T_rl.m[i] = pose0[12 + i]; }
            p.dev_pose = first_eval ? nullptr : st->pose;
            hipLaunchKernelGGL(k_icp_point_plane, dim3(g.gx, g.gy), dim3(g.bx, g.by), g.lds_bytes, s, p);
            hipLaunchKernelGGL(k_lss_final_solve, dim3(1), dim3(256), 0, s, sums, (int)g.blocks, st, L.rotation_only ? 1 : 0, max_rmse, kn, first_eval ? 1 : 0,
                               last ? (double*)mail : nullptr, seq);
        }
    }
    if (int e = check_launch("kfx_icp_refine")) return e;
    if (mail) {
        if (enqueue_more) enqueue_more(user);
        if (result_port.wait_mailbox(seq, s)) {
            deliver((const double*)result_port.mail, T_lp, rmse, obs, tracking_good);
            return 0;
        }
    }
    return copy_result(mail ? nullptr : enqueue_more);
}

extern "C" int kfx_icp_refine(const kfx_icp_level* levels, int n_levels, float c, float max_rmse, const kfx_image* workspace,
                              const kfx_image* debug, double T_lp[12], float* rmse, unsigned* obs, int* tracking_good, kfx_stream stream)
{
    return icp_refine_impl(levels, n_levels, c, max_rmse, workspace, debug, T_lp, rmse, obs, tracking_good, nullptr, nullptr, stream);
}

// kfx_icp_refine with a hook between enqueueing the pose's read-back and waiting for it (include/kfx.h)
extern "C" int kfx_icp_refine_then(const kfx_icp_level* levels, int n_levels, float c, float max_rmse, const kfx_image* workspace,
                                   const kfx_image* debug, double T_lp[12], float* rmse, unsigned* obs, int* tracking_good,
                                   void (*enqueue_more)(void* user), void* user, kfx_stream stream)
{
    return icp_refine_impl(levels, n_levels, c, max_rmse, workspace, debug, T_lp, rmse, obs, tracking_good, enqueue_more, user, stream);
}
