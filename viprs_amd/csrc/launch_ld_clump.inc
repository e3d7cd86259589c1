// Host-side launcher of the clumping kernel (ld_clump.h) for one LD element type:
//     #define CLUMP_U      the LD element type
//     #define CLUMP_DENSE  0 / 1: the element type has repacked dense blocks (the types the panel schedule accepts)
// then include.  The order pieces, the thresholds, the masks and the output are the plan's buffers (abi_clump.hip).
#include "internal.h"
#include "ld_clump.h"

namespace viprs {
namespace {
viprs::BuildFlagsRegistrar tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

// one workgroup per block of blocks[block0 .. block0 + n_blocks)
template <typename U, int MODE>
int launch_blocks(viprs_plan* P, ClumpArgs A, int block0, size_t n_blocks) {
    if (n_blocks == 0) return VIPRS_OK;
    A.block0 = block0;
    ld_clump_kernel<U, MODE><<<dim3((unsigned)n_blocks), dim3(kClumpThreads), 0, P->stream>>>(A);
    HIP_TRY(hipGetLastError());
    return VIPRS_OK;
}
}  // namespace

template <>
int launch_ld_clump<CLUMP_U>(viprs_plan* P, int n_cols) {
    ClumpArgs A;
    A.blocks = P->d_dot_blocks.p;
    A.rows = nullptr;
    A.n_rows = 0;
    A.ip = P->d_ip.p;
    A.lb = P->d_lb.p;
    A.first = P->d_dot_first.p;
    A.m = P->m;
    A.order = P->d_clump_order.p;
    A.order_off = P->d_clump_off.p;
    A.thr = P->d_clump_thr.p;
    A.n_cols = n_cols;
    A.mask = P->d_clump_mask.p;
    A.index_of = P->d_clump_index.p;
    const size_t n_dense = P->dense_all_h.size(), n_ragged = P->ragged_all_h.size();
    int rc = VIPRS_OK;
#if CLUMP_DENSE
    A.ld = P->d_ld_dense.p;
    // upper form: whole rows from the mirrored squares; the float64 sweeps' zero lower triangle is read as it is
    if (!P->low_memory || P->mirror) rc = launch_blocks<CLUMP_U, kDotDense>(P, A, 0, n_dense);
    else rc = launch_blocks<CLUMP_U, kDotDenseGather>(P, A, 0, n_dense);
    if (rc != VIPRS_OK) return rc;
#else
    if (n_dense != 0) return fail(VIPRS_EUNSUPPORTED, "dense blocks of an LD element type without repacked squares");
#endif
    A.ld = P->d_ld_raw.p;
    if (P->low_memory) rc = launch_blocks<CLUMP_U, kDotWindowUpper>(P, A, (int)n_dense, n_ragged);
    else rc = launch_blocks<CLUMP_U, kDotWindowSym>(P, A, (int)n_dense, n_ragged);
    return rc;
}

}  // namespace viprs
