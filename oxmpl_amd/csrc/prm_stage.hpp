// prm_stage.hpp -- how PRM's construction kernels append what they find, in both spaces (prm_kernels.hip, prm_so3.hip):
// the pair search's per-wave staging of candidates, and the edge kernels' two directed keys per valid motion.
#pragma once
#include "oxhip_internal.hpp"
#include "rrt_device.hpp"

namespace oxhip {

constexpr int kStage = 512;                         // per-wave LDS staging of hits before they go to HBM

// Hits are appended to a per-wave LDS buffer with ballot / prefix-count positions (the wave is its only
// writer, so no atomic is involved) and flushed to the candidate list with ONE global atomic per flush.
// A single global counter bumped once per hit serialises at the L2: 291 k hits cost 3 ms that way.
struct PairStage {
    uint2* buf;       // this wave's kStage entries in LDS
    uint32_t cnt;     // wave-uniform
};

__device__ __forceinline__ void stage_flush(const PrmArgs& a, PairStage& st, uint32_t lane) {
    if (st.cnt == 0) return;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&a.state->n_cand, (unsigned long long)st.cnt);
    base = uni64(base);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's LDS writes precede its reads below
    for (uint32_t e = lane; e < st.cnt; e += 64) {
        const unsigned long long slot = base + e;
        if (slot < (unsigned long long)a.cand_cap) a.cand[slot] = st.buf[e];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and those reads precede the next writes
    st.cnt = 0;
}

// the end of an edge kernel: both directed keys of every lane whose motion (j -> i) is valid.
// One atomic per wave: a counter bumped once per edge serialises at the L2.
__device__ __forceinline__ void append_edge_keys(bool ok, uint32_t j, uint32_t i, uint64_t* keys, uint32_t* n_keys, uint32_t key_shift,
                                                 uint32_t lane) {
    const uint64_t bal = __ballot(ok);
    if (bal == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(n_keys, 2u * (uint32_t)__popcll(bal));
    base = uni(base);
    if (ok) {
        const uint32_t slot = base + 2u * (uint32_t)__popcll(bal & below_mask(lane));
        keys[slot] = ((uint64_t)j << key_shift) | i;       // i in j's list
        keys[slot + 1] = ((uint64_t)i << key_shift) | j;   // j in i's list (prm.rs:143-145)
    }
}

}  // namespace oxhip
