// Batched grid E-step on the matrix cores (estep_grid_mfma.h) for one LD element type: included by
// grid_f32.hip / grid_i8.hip / grid_i16.hip with GRID_U defined.
#include "internal.h"
#include "estep_grid_mfma.h"

static viprs::BuildFlagsRegistrar viprs_tu_build_flags_(VIPRS_TU_BUILD_FLAGS);

namespace viprs {

// Batched grid E-step on the matrix cores: every LD row is read once for up to 32 models.
template <typename U>
int launch_grid_mfma(viprs_plan* P, EStepArgs<float> A) {
    A.blocks = P->d_dense.p;
    A.n_blocks = (int)P->dense_h.size();
    A.counter = P->d_counters.p + 12;
    const size_t shmem = (size_t)kGridLdsFloats * sizeof(float);
    const bool exact = P->math_mode == VIPRS_MATH_EXACT;      // fast: the chain's sigmoid on v_exp_f32 / v_rcp_f32
    // upper-triangular form: the sweep runs over the MIRRORED storage and carries the second pass itself (grid_block_resident)
    // (grouped: a grid state with a (group, column) mask -- per-block model lists, estep_grid_mfma.h)
    const void* kfn = A.group_lists
        ? (P->low_memory
           ? (exact ? (const void*)estep_grid_mfma_kernel<U, false, true, true> : (const void*)estep_grid_mfma_kernel<U, false, false, true>)
           : (exact ? (const void*)estep_grid_mfma_kernel<U, true, true, true> : (const void*)estep_grid_mfma_kernel<U, true, false, true>))
        : (P->low_memory
           ? (exact ? (const void*)estep_grid_mfma_kernel<U, false, true> : (const void*)estep_grid_mfma_kernel<U, false, false>)
           : (exact ? (const void*)estep_grid_mfma_kernel<U, true, true> : (const void*)estep_grid_mfma_kernel<U, true, false>));
    P->math_used |= exact ? 1 : 2;
    HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, 64 * kGridWaves, shmem));
    const int capacity = P->n_cu * std::max(1, per_cu);          // workgroups resident at once
    if (P->low_memory) { const int rc = ensure_upper_storage(P, true); if (rc != VIPRS_OK) return rc; }
    // Blocks whose q fits the updater waves' accumulators (<= kGridResMaxCols SNPs) take one workgroup each, from a queue.
    // Blocks beyond that: TEAMS of ceil(tiles / 12) workgroups, each member resident on its own tiles, the chain migrating
    // from member to member (estep_grid_mfma.h, GridTeam).  Every member of every team of a launch has to be resident (the
    // team workgroups are the head of the grid): the first launch takes as many of the LARGEST blocks as fit half the chip --
    // the other half starts on the queue of the remaining blocks at once --, team blocks left over follow in further launches
    // of team workgroups only, a chipful at a time.
    if (!P->grid_teams_built) {
        std::vector<int32_t> blk, mem, siz;
        std::vector<int64_t> goff;
        int64_t g = 0;
        int nb = 0;
        while (nb < (int)P->dense_h.size() && P->dense_h[(size_t)nb].size > kGridResMaxCols) {
            const int b = P->dense_h[(size_t)nb].size;
            const int tiles = (b + 2 * kPanel - 1) / (2 * kPanel);
            const int ts = (tiles + kGridResOwners * kGridResSlots - 1) / (kGridResOwners * kGridResSlots);
            for (int m = 0; m < ts; ++m) { blk.push_back(nb); mem.push_back(m); siz.push_back(ts); }
            goff.push_back(g);
            g += (int64_t)((b + kPanel - 1) / kPanel) * kGridAFloats;
            ++nb;
        }
        P->grid_team_blocks = nb;
        P->grid_team_wgs = (int)blk.size();
        P->grid_team_ts.clear();
        for (int i = 0, w = 0; i < nb; ++i) { P->grid_team_ts.push_back(siz[(size_t)w]); w += siz[(size_t)w]; }
        if (nb > 0) {
            HIP_TRY(hipStreamSynchronize(P->stream));             // (a rebuild after viprs_plan_set_active_blocks: nothing in flight)
            HIP_TRY(P->d_grid_team_block.alloc(blk.size()));
            HIP_TRY(P->d_grid_team_member.alloc(mem.size()));
            HIP_TRY(P->d_grid_team_size.alloc(siz.size()));
            HIP_TRY(P->d_grid_team_goff.alloc(goff.size()));
            HIP_TRY(hipMemcpy(P->d_grid_team_block.p, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(P->d_grid_team_member.p, mem.data(), mem.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(P->d_grid_team_size.p, siz.data(), siz.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(P->d_grid_team_goff.p, goff.data(), goff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            HIP_TRY(P->d_grid_gran.alloc((size_t)g));
            HIP_TRY(hipMemset(P->d_grid_gran.p, 0, (size_t)g * sizeof(unsigned long long)));
            P->grid_gen = 0;
        }
        P->grid_teams_built = true;
    }
    const int n_team_blocks = P->grid_team_blocks;
    const int n_queue = A.n_blocks - n_team_blocks;
    int tb0 = 0, wg0 = 0;                                         // first team block / team workgroup of the coming launch
    bool first = true;
    while (first || tb0 < n_team_blocks) {
        // the first launch: teams on at most half the chip when there is a queue to work on beside them; later ones: teams only
        const int budget = (first && n_queue > 0) ? std::max(1, capacity / 2) : capacity;
        int n_tb = 0, n_twg = 0;
        while (tb0 + n_tb < n_team_blocks && n_twg + P->grid_team_ts[(size_t)(tb0 + n_tb)] <= budget) {
            n_twg += P->grid_team_ts[(size_t)(tb0 + n_tb)];
            ++n_tb;
        }
        if (tb0 < n_team_blocks && n_tb == 0) return fail(VIPRS_EUNSUPPORTED, "a grid team exceeds the resident workgroups of the device");
        GridTeams T{};
        if (n_tb > 0) {
            P->grid_gen = (P->grid_gen + 1) & 0xFFFFFu;
            if (P->grid_gen == 0) {                                // tags wrap: clear once every 2^20 launches
                HIP_TRY(hipMemsetAsync(P->d_grid_gran.p, 0, P->d_grid_gran.n * sizeof(unsigned long long), P->stream));
                P->grid_gen = 1;
            }
            T.n_wgs = n_twg;
            T.n_blocks = n_tb;
            T.block = P->d_grid_team_block.p + wg0;               // (absolute indices into the size-sorted block list)
            T.member = P->d_grid_team_member.p + wg0;
            T.size = P->d_grid_team_size.p + wg0;
            T.goff = P->d_grid_team_goff.p;
            T.gran = P->d_grid_gran.p;
            T.tag_base = P->grid_gen << 12;
        }
        // the queue (blocks behind the team blocks of the PLAN) belongs to the first launch
        T.queue_start = first ? n_team_blocks : A.n_blocks;
        const int grid = std::min<int>(capacity, n_twg + (first ? n_queue : 0));
        if (grid > 0) {
            void* params[] = {(void*)&A, (void*)&T};
            if (n_tb > 0) { const int rc = team_launch_gate(P); if (rc != VIPRS_OK) return rc; }
            { const int rc = P->timing.launcher_start(); if (rc != VIPRS_OK) return rc; }      // (first launch of the sweep only: cleared after)
            HIP_TRY(hipLaunchKernel(kfn, dim3(grid), dim3(64 * kGridWaves), params, shmem, P->stream));
            if (n_tb > 0) { const int rc = team_launch_done(P); if (rc != VIPRS_OK) return rc; }
        }
        tb0 += n_tb;
        wg0 += n_twg;
        first = false;
    }
    return P->timing.launcher_start();           // (nothing was launched: an empty schedule)
}

template int launch_grid_mfma<GRID_U>(viprs_plan*, EStepArgs<float>);

}  // namespace viprs
