// rrt_so2_services.hip -- the batch-level services of an SO(2) RRT batch (OXHIP_SPACE_SO2): the SO(2) instantiations, SeqSpace<-1>, of
// the kernels that are written once over the space -- the re-check's edge, compaction and skip kernels (rrt_reval_kernels.hpp,
// DESIGN.md section 21) and the shortcutter's pair matrix and DP (path_kernels.hpp) -- and their launchers,
// which rrt_revalidate.hip and path_simplify.hip call for this space.
#include "oxhip_internal.hpp"
#include "path_kernels.hpp"
#include "rrt_reval_kernels.hpp"

namespace oxhip {

void launch_so2_reval_edges(const DevParams& p, const RevalArgs& a, uint32_t n_problems, hipStream_t s) {
    hipLaunchKernelGGL(rrt_reval_edge_kernel<-1>, dim3(n_problems * a.tiles), dim3(256), 0, s, SeqSpace<-1>::checker(p), a);
}
void launch_so2_reval_compact(const RevalArgs& a, uint32_t n_problems, hipStream_t s) {
    hipLaunchKernelGGL(rrt_reval_compact_kernel<-1>, dim3(n_problems), dim3(256), 0, s, a);
    hipLaunchKernelGGL(rrt_reval_skip_kernel<-1>, dim3(n_problems * a.tiles), dim3(256), 0, s, a);
}
void launch_so2_path_pairs(const DevParams& p, const PairArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(path_pairs_kernel<-1>, dim3((uint32_t)((a.n_words + 3u) / 4u)), dim3(256), 0, s, SeqSpace<-1>::checker(p), a);
}
void launch_so2_path_dp(const PairArgs& a, const SimplifyOut& o, hipStream_t s) {
    hipLaunchKernelGGL(path_dp_kernel<2>, dim3(a.n_chunk), dim3(64), 0, s, a, o, 1u);
}

}  // namespace oxhip
