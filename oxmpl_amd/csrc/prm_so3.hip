// prm_so3.hip -- PRM (oxmpl/src/geometric/planners/prm.rs) over SO3StateSpace with forbidden cones, on gfx950 (wave64).
//
// The phases of prm_kernels.hip with SO(3) operations (so3_device.hpp):
//   1. prm_so3_sample_spec_kernel / _scan_kernel / _compact_kernel
//        sample_uniform (so3_state_space.rs:201-231) is a rejection loop of four random_range(-1.0..1.0) words per attempt.
//        That range never redraws, so attempt a of a round sits at stream words pos0 + 4a .. pos0 + 4a + 3 and every attempt
//        is evaluated side by side: "accepted" (a sample_uniform call returned) and "accepted and valid" (a milestone) are
//        ballots, a scan finds where the round ends (the roadmap is full or max_samples calls were made) and a compaction
//        appends the milestones in order.  max_angle < 1e-9: every attempt is the centre and draws no word.
//   2. prm_so3_pairs_kernel   all pairs (j, i < j): 4 register-resident j per thread, the i quaternion one scalar 32-byte load;
//        the reference's binary64 dot (4 mul + 3 add, unfused), then distance < r decided by bands of |dot| computed on the
//        host (above hi: in, below lo: out, in between: so3_distance itself, ox_acos included)
//   3. prm_so3_edge_kernel    check_motion(m_j -> m_i) per candidate (so3_interpolate), cones in LDS; both directed keys
// The query sets are prm_kernels.hip's prm_query_kernel over SeqSpace<0> (seq_space.hpp).
// The keys go through prm_kernels.hip's sort and CSR extraction, so every node's `edges` list ends up ascending.
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"
#include "so3_device.hpp"
#include "prm_stage.hpp"
#include "seq_space.hpp"

namespace oxhip {

// ------------------------------------------------------------------------------------------------
// 1. sampling

constexpr int kSo3SpecThreads = 256;

__global__ __launch_bounds__(kSo3SpecThreads) void prm_so3_sample_spec_kernel(DevParams p, PrmArgs a, PrmSo3Spec sp) {
    constexpr int kBlocks = kSo3SpecThreads * 4 / 8 + 2;   // the workgroup's 4 * 256 words start anywhere in a block
    __shared__ uint32_t wbuf[kBlocks][16];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t s0 = blockIdx.x * kSo3SpecThreads;
    const uint32_t s = s0 + tid;
    const bool act = s < sp.m;
    double q[4] = {p.so3_centre[0], p.so3_centre[1], p.so3_centre[2], p.so3_centre[3]};
    bool acc = act, redraw = false;
    if (!(p.so3_max_angle < 1e-9)) {   // (workgroup-uniform) otherwise: the centre, no word drawn (so3_state_space.rs:204-206)
        const uint64_t w0 = sp.pos0 + (uint64_t)s0 * 4u;
        const uint64_t blk0 = w0 >> 3;
        for (uint32_t b = tid; b < (uint32_t)kBlocks; b += kSo3SpecThreads) {
            uint32_t o[16];
            chacha12_block(p.seed, blk0 + b, a.stream, o);
#pragma unroll
            for (int w = 0; w < 16; ++w) wbuf[b][w] = o[w];
        }
        __syncthreads();
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t rel = (uint32_t)(w0 - (blk0 << 3)) + tid * 4u + (uint32_t)k;   // < kBlocks * 8
            const uint64_t word = ((uint64_t)wbuf[rel >> 3][(rel & 7) * 2 + 1] << 32) | wbuf[rel >> 3][(rel & 7) * 2];
            redraw = redraw || !so3_range_word(word, v[k]);
        }
        acc = act && !redraw && so3_attempt(v, p.so3_centre, p.so3_max_angle, q);
    }
    if (__ballot(act && redraw) != 0 && lane == 0) atomicOr(sp.redraw_flag, 1u);
    const bool valid = acc && !so3_cone_hit(p.sph_c, p.n_spheres, p.sph_r, p.n_spheres, q);   // prm.rs:123
    const uint64_t vb = __ballot(valid), ab = __ballot(acc);
    if (valid) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sp.tmp[(size_t)s * 4 + k] = q[k];
    }
    if (lane == 0 && s < sp.m) {   // (a wave wholly beyond the round has no slot)
        sp.vbits[s >> 6] = vb;
        sp.abits[s >> 6] = ab;
        sp.voff[s >> 6] = (uint32_t)__popcll(vb);
        sp.acnt[s >> 6] = (uint32_t)__popcll(ab);
    }
}

__device__ __forceinline__ uint32_t nth_set_bit(uint64_t bits, uint32_t n) {   // index of the n-th (1-based) set bit
    for (uint32_t k = 1; k < n; ++k) bits &= bits - 1;
    return (uint32_t)(__ffsll((unsigned long long)bits) - 1);
}

__device__ __forceinline__ uint64_t upto_mask(uint32_t l) { return l >= 63u ? ~0ull : (2ull << l) - 1ull; }

// one workgroup: exclusive scans of the per-wave milestone and sample counts; the round ends after the attempt that completes the
// roadmap (the need_v-th milestone) or that makes the max_samples-th sample_uniform call (the need_a-th accepted attempt)
__global__ __launch_bounds__(1024) void prm_so3_sample_scan_kernel(PrmArgs a, PrmSo3Spec sp, uint32_t words_per_attempt) {
    __shared__ uint32_t wsv[16], wsa[16];
    __shared__ uint32_t cut_v, cut_v_acc, cut_a, cut_a_val;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nw = (sp.m + 63) >> 6;
    const uint32_t per = (nw + 1023) / 1024;
    const uint32_t b = tid * per < nw ? tid * per : nw, e = b + per < nw ? b + per : nw;
    uint32_t mv = 0, ma = 0;
    for (uint32_t w = b; w < e; ++w) { mv += sp.voff[w]; ma += sp.acnt[w]; }
    uint32_t iv = mv, ia = ma;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t ov = __shfl_up(iv, off, 64), oa = __shfl_up(ia, off, 64);
        if ((int)lane >= off) { iv += ov; ia += oa; }
    }
    if (lane == 63) { wsv[wave] = iv; wsa[wave] = ia; }
    if (tid == 0) { cut_v = cut_a = 0xFFFFFFFFu; cut_v_acc = cut_a_val = 0; }
    __syncthreads();
    uint32_t bv = 0, ba = 0, tv = 0, ta = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        bv += (uint32_t)w < wave ? wsv[w] : 0u;
        ba += (uint32_t)w < wave ? wsa[w] : 0u;
        tv += wsv[w];
        ta += wsa[w];
    }
    uint32_t rv = bv + iv - mv, ra = ba + ia - ma;
    const PrmState st = *a.state;
    const uint32_t need_v = a.n_target - st.n_milestones;                      // > 0: the host only launches an open round
    const uint64_t left = a.max_samples - st.n_samples;                       // > 0 likewise
    const uint32_t need_a = left < 0xFFFFFFFFull ? (uint32_t)left : 0xFFFFFFFFu;
    for (uint32_t w = b; w < e; ++w) {
        const uint32_t cv = sp.voff[w], ca = sp.acnt[w];
        sp.voff[w] = rv;
        if (rv < need_v && rv + cv >= need_v) {
            const uint32_t l = nth_set_bit(sp.vbits[w], need_v - rv);
            cut_v = w * 64 + l;
            cut_v_acc = ra + (uint32_t)__popcll(sp.abits[w] & upto_mask(l));
        }
        if (ra < need_a && ra + ca >= need_a) {
            const uint32_t l = nth_set_bit(sp.abits[w], need_a - ra);
            cut_a = w * 64 + l;
            cut_a_val = rv + (uint32_t)__popcll(sp.vbits[w] & upto_mask(l));
        }
        rv += cv;
        ra += ca;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t consumed = sp.m, dv = tv, da = ta;
        if (cut_v != 0xFFFFFFFFu && cut_v <= cut_a) { consumed = cut_v + 1; dv = need_v; da = cut_v_acc; }
        else if (cut_a != 0xFFFFFFFFu) { consumed = cut_a + 1; dv = cut_a_val; da = need_a; }
        PrmState ns = st;
        ns.n_milestones = st.n_milestones + dv;
        ns.n_samples = st.n_samples + da;
        ns.draws = st.draws + (uint64_t)consumed * words_per_attempt;
        sp.result[0] = ns;
    }
}

// ordered compaction of the round's milestones behind the existing ones (those after the round's end are dropped)
__global__ __launch_bounds__(kSo3SpecThreads) void prm_so3_sample_compact_kernel(PrmArgs a, PrmSo3Spec sp, uint32_t n0) {
    const uint32_t s = blockIdx.x * kSo3SpecThreads + threadIdx.x, lane = threadIdx.x & 63;
    if (s >= sp.m) return;
    const uint64_t bal = sp.vbits[s >> 6];
    if (!((bal >> lane) & 1ull)) return;
    const uint32_t dst = n0 + sp.voff[s >> 6] + (uint32_t)__popcll(bal & below_mask(lane));
    if (dst >= sp.result->n_milestones) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.ms[(size_t)dst * 4 + k] = sp.tmp[(size_t)s * 4 + k];
}

// ------------------------------------------------------------------------------------------------
// 2. all pairs within the connection radius

constexpr int kSo3PairThreads = 256;
constexpr int kSo3PairR = 4;                                   // milestones j held in registers per thread
constexpr int kSo3PairJB = kSo3PairThreads * kSo3PairR;        // j per workgroup
constexpr int kSo3PairIC = 256;                                // i per workgroup
                                                               // (the hits' staging in LDS and its flush: prm_stage.hpp)

template <bool DIAG>
__device__ __forceinline__ void so3_pairs_range(const PrmArgs& a, PairStage& st, uint32_t lane, const double (&cj)[kSo3PairR][4],
                                                const uint32_t (&jr)[kSo3PairR], const double* __restrict__ ms, uint32_t lo_i,
                                                uint32_t hi_i, double lo, double hi, double r) {
    for (uint32_t i = lo_i; i < hi_i; ++i) {
        const double ci[4] = {ms[(size_t)i * 4], ms[(size_t)i * 4 + 1], ms[(size_t)i * 4 + 2], ms[(size_t)i * 4 + 3]};   // wave-uniform
        double ad[kSo3PairR];
        bool in[kSo3PairR], band[kSo3PairR];
        bool any_band = false, any_in = false;
#pragma unroll
        for (int q = 0; q < kSo3PairR; ++q) {
            ad[q] = fabs(so3_dot(cj[q], ci));   // distance(q_new, m_i): the reference's dot, unfused
            in[q] = ad[q] > hi;
            band[q] = !in[q] && ad[q] >= lo;    // (NaN of an empty slot: neither)
            if (DIAG) { in[q] = in[q] && i < jr[q]; band[q] = band[q] && i < jr[q]; }
            any_band = any_band || band[q];
            any_in = any_in || in[q];
        }
        if (__ballot(any_band) != 0) {
#pragma unroll
            for (int q = 0; q < kSo3PairR; ++q) {
                if (band[q]) {
                    const double d = ad[q] > 1.0 - 1e-9 ? 0.0 : ox_acos(ad[q]);   // so3_state_space.rs:101-110
                    in[q] = d < r;                                                 // prm.rs:134 (strict)
                    any_in = any_in || in[q];
                }
            }
        }
        if (__ballot(any_in) != 0) {
#pragma unroll
            for (int q = 0; q < kSo3PairR; ++q) {
                const uint64_t m = __ballot(in[q]);
                if (in[q]) st.buf[st.cnt + (uint32_t)__popcll(m & below_mask(lane))] = make_uint2(jr[q], i);
                st.cnt += (uint32_t)__popcll(m);
            }
            if (st.cnt > (uint32_t)(kStage - 64 * kSo3PairR)) stage_flush(a, st, lane);   // room for one more i
        }
    }
}

__global__ __launch_bounds__(kSo3PairThreads) void prm_so3_pairs_kernel(PrmArgs a, const double* __restrict__ ms, uint32_t j0, uint32_t j1,
                                                                         double lo, double hi, double r) {
    __shared__ uint2 stage[kSo3PairThreads / 64][kStage];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t jb0 = j0 + blockIdx.y * kSo3PairJB;
    const uint32_t jb1 = jb0 + kSo3PairJB < j1 ? jb0 + kSo3PairJB : j1;
    const uint32_t i_lo = blockIdx.x * kSo3PairIC;
    if (jb0 >= j1 || i_lo + 1 >= jb1) return;
    const uint32_t i_hi = i_lo + kSo3PairIC < jb1 - 1 ? i_lo + kSo3PairIC : jb1 - 1;
    double cj[kSo3PairR][4];   // a slot beyond the range holds NaN: its |dot| is neither above hi nor in the band
    uint32_t jr[kSo3PairR];
#pragma unroll
    for (int q = 0; q < kSo3PairR; ++q) {
        jr[q] = jb0 + q * kSo3PairThreads + tid;
#pragma unroll
        for (int k = 0; k < 4; ++k) cj[q][k] = jr[q] < jb1 ? ms[(size_t)jr[q] * 4 + k] : __builtin_nan("");
    }
    PairStage st{stage[tid >> 6], 0u};
    const uint32_t i_mid = i_hi < jb0 ? i_hi : (i_lo > jb0 ? i_lo : jb0);
    so3_pairs_range<false>(a, st, lane, cj, jr, ms, i_lo, i_mid, lo, hi, r);
    so3_pairs_range<true>(a, st, lane, cj, jr, ms, i_mid, i_hi, lo, hi, r);
    stage_flush(a, st, lane);
}

// ------------------------------------------------------------------------------------------------
// 3. check_motion per candidate pair (from = the newer milestone j, to = the older one i: prm.rs:134)

constexpr int kSo3LdsCones = 64;

template <bool LDS_CONES>
__global__ __launch_bounds__(256) void prm_so3_edge_kernel(So3Cones p, const uint2* __restrict__ cand, const double* __restrict__ ms,
                                                            uint64_t* __restrict__ keys, uint32_t* n_keys, uint32_t n_cand, uint32_t key_shift) {
    __shared__ double cone_c[4][LDS_CONES ? kSo3LdsCones : 1];
    __shared__ double cone_r[LDS_CONES ? kSo3LdsCones : 1];
    const uint32_t c = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const uint32_t nc = p.n;
    const double* cc = p.c;
    const double* cr = p.r;
    uint32_t stride = nc;
    if (LDS_CONES) {
        for (uint32_t j = threadIdx.x; j < nc; j += 256) {
#pragma unroll
            for (int k = 0; k < 4; ++k) cone_c[k][j] = p.c[(size_t)k * nc + j];
            cone_r[j] = p.r[j];
        }
        __syncthreads();
        cc = &cone_c[0][0];
        cr = cone_r;
        stride = (uint32_t)kSo3LdsCones;
    }
    bool ok = false;
    uint2 pr = make_uint2(0u, 0u);
    if (c < n_cand) {
        pr = cand[c];
        double from[4], to[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            from[k] = ms[(size_t)pr.x * 4 + k];
            to[k] = ms[(size_t)pr.y * 4 + k];
        }
        ok = so3_motion_valid_seq(cc, stride, cr, nc, from, to, p.res);
    }
    append_edge_keys(ok, pr.x, pr.y, keys, n_keys, key_shift, lane);
}

// ------------------------------------------------------------------------------------------------
// launchers

void launch_prm_so3_sample(const DevParams& p, const PrmArgs& a, const PrmSo3Spec& sp, uint32_t n0, hipStream_t s) {
    const uint32_t blocks = (sp.m + kSo3SpecThreads - 1) / kSo3SpecThreads;
    const uint32_t wpa = p.so3_max_angle < 1e-9 ? 0u : 4u;
    hipLaunchKernelGGL(prm_so3_sample_spec_kernel, dim3(blocks), dim3(kSo3SpecThreads), 0, s, p, a, sp);
    hipLaunchKernelGGL(prm_so3_sample_scan_kernel, dim3(1), dim3(1024), 0, s, a, sp, wpa);
    hipLaunchKernelGGL(prm_so3_sample_compact_kernel, dim3(blocks), dim3(kSo3SpecThreads), 0, s, a, sp, n0);
}

void launch_prm_so3_pairs(const PrmArgs& a, uint32_t j0, uint32_t j1, double lo, double hi, double r, hipStream_t s) {
    if (j1 <= j0 || j1 < 2) return;
    const uint32_t jblocks = (j1 - j0 + kSo3PairJB - 1) / kSo3PairJB;
    const uint32_t ichunks = (j1 - 1 + kSo3PairIC - 1) / kSo3PairIC;
    hipLaunchKernelGGL(prm_so3_pairs_kernel, dim3(ichunks, jblocks), dim3(kSo3PairThreads), 0, s, a, (const double*)a.ms, j0, j1, lo, hi, r);
}

void launch_prm_so3_edges(const DevParams& p, const PrmArgs& a, uint32_t n_cand, hipStream_t s) {
    if (n_cand == 0) return;
    const uint32_t shift = prm_key_shift(a.cap);
    const So3Cones cones = SeqSpace<0>::checker(p);
    uint32_t* n_keys = &a.state->n_keys;
    if (p.n_spheres <= (uint32_t)kSo3LdsCones)
        hipLaunchKernelGGL(prm_so3_edge_kernel<true>, dim3((n_cand + 255) / 256), dim3(256), 0, s, cones, (const uint2*)a.cand,
                           (const double*)a.ms, a.keys, n_keys, n_cand, shift);
    else
        hipLaunchKernelGGL(prm_so3_edge_kernel<false>, dim3((n_cand + 255) / 256), dim3(256), 0, s, cones, (const uint2*)a.cand,
                           (const double*)a.ms, a.keys, n_keys, n_cand, shift);
}

}  // namespace oxhip
