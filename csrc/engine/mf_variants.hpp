// The kernel variants of the multi-frame MFMA projections: one list per kernel signature, one entry per
// instantiation. The planner's table of supported keys (mf_plan.cpp) and the kernel tables of multiframe.hip /
// multiframe_bf16.hip are generated from these lists (keys: mf_key_* in mf_plan.hpp, argument for argument).
//
// What is listed:
//   (a) every key the planner returns with no knob set, for any supported nf, ld and padded row count;
//   (b) every key reached by a knob setting named in tests/ (the parametrisations of test_gpu_multiframe_bf16.py,
//       mf_set_rows / mf_set_vox in test_gpu_kernels.py) or swept by tools/probe_mf.py (depth x rows / vox);
//   (c) each A/B knob alone against the defaults: SART_MF_DEPTH, SART_MF_ROWS, SART_MF_VOX, SART_MF_NT, the tiles of
//       (b) for SART_MF_B16_FWD / SART_MF_X3_FWD, SART_MF_B16_VT, SART_MF_X3_DEPTH, SART_MF_X3_VT, SART_MF_XEARLY,
//       SART_MF_WEARLY, SART_MF_H16 = ew / w1 / ew,w1, SART_MF_H16_FDEPTH=3.
// Nothing else: a combination of knobs that needs another instantiation throws in the planner. To try one, add its
// line here.
#pragma once

// forward, fp32 MFMA: k_mf_forward<NG, DEPTH, RT, NT>
#define MF_FWD_F32_VARIANTS(X) \
    X(1, 1, 2, 0) X(1, 1, 4, 0) X(1, 2, 2, 0) X(1, 2, 4, 0) X(1, 3, 2, 0) X(1, 3, 2, 1) \
    X(1, 3, 4, 0) X(1, 3, 4, 1) X(2, 1, 2, 0) X(2, 1, 4, 0) X(2, 2, 2, 0) X(2, 2, 4, 0) \
    X(2, 3, 2, 0) X(2, 3, 2, 1) X(2, 3, 4, 0) X(2, 3, 4, 1) X(4, 1, 2, 0) X(4, 1, 4, 0) \
    X(4, 2, 2, 0) X(4, 2, 2, 1) X(4, 2, 4, 0) X(4, 2, 4, 1) X(4, 3, 2, 0) X(4, 3, 4, 0)

// forward, bf16 storage: X(LDS, NG, DEPTH, RT, KB, AS, EX). LDS 0: k_mf_forward_b16<NG, DEPTH, RT, KB>;
// LDS 1: k_mf_forward_b16_lds<NG, DEPTH, RT, KB, bf16_t, AS, EX>
#define MF_FWD_B16_VARIANTS(X) \
    X(0, 1, 3, 2, 1, 0, 0) X(0, 1, 3, 4, 1, 0, 0) X(0, 1, 3, 8, 1, 0, 0) X(0, 2, 3, 2, 1, 0, 0) X(0, 2, 3, 4, 1, 0, 0) \
    X(0, 2, 3, 8, 1, 0, 0) X(0, 4, 3, 2, 1, 0, 0) X(0, 4, 3, 4, 1, 0, 0) X(0, 4, 3, 8, 1, 0, 0) X(1, 1, 1, 2, 2, 0, 0) \
    X(1, 1, 2, 2, 2, 0, 0) X(1, 1, 3, 2, 1, 0, 0) X(1, 1, 3, 2, 2, 0, 0) X(1, 1, 3, 2, 2, 0, 1) X(1, 1, 3, 2, 2, 1, 0) \
    X(1, 1, 3, 4, 2, 0, 0) X(1, 1, 3, 4, 2, 1, 0) X(1, 1, 3, 8, 1, 0, 0) X(1, 2, 1, 2, 2, 1, 0) X(1, 2, 2, 2, 2, 1, 0) \
    X(1, 2, 3, 2, 1, 0, 0) X(1, 2, 3, 2, 2, 0, 0) X(1, 2, 3, 2, 2, 1, 0) X(1, 2, 3, 2, 2, 1, 1) X(1, 2, 3, 4, 2, 0, 0) \
    X(1, 2, 3, 4, 2, 1, 0) X(1, 2, 3, 8, 1, 0, 0) X(1, 4, 1, 2, 1, 0, 0) X(1, 4, 1, 4, 2, 0, 0) X(1, 4, 2, 2, 1, 0, 0) \
    X(1, 4, 2, 4, 2, 0, 0) X(1, 4, 3, 2, 1, 0, 0) X(1, 4, 3, 2, 1, 0, 1) X(1, 4, 3, 2, 2, 0, 0) X(1, 4, 3, 2, 2, 1, 0) \
    X(1, 4, 3, 4, 2, 0, 0) X(1, 4, 3, 4, 2, 0, 1) X(1, 4, 3, 4, 2, 1, 0) X(1, 4, 3, 8, 1, 0, 0) X(1, 8, 2, 2, 2, 1, 0) \
    X(1, 8, 3, 2, 2, 1, 0)

// forward, split-A: X(H16, NG, DEPTH, RT, KB, AS, EX): k_mf_forward_b16_lds<NG, DEPTH, RT, KB, float, AS, EX, H16>
#define MF_FWD_A32_VARIANTS(X) \
    X(0, 1, 2, 2, 1, 0, 1) X(0, 1, 2, 2, 1, 1, 1) X(0, 1, 2, 2, 2, 0, 0) X(0, 1, 2, 2, 2, 0, 1) X(0, 1, 2, 2, 2, 1, 1) \
    X(0, 1, 2, 4, 1, 1, 1) X(0, 1, 2, 4, 2, 0, 1) X(0, 1, 3, 2, 1, 0, 1) X(0, 1, 3, 2, 2, 0, 1) X(0, 1, 3, 2, 2, 1, 1) \
    X(0, 1, 3, 4, 2, 0, 1) X(0, 2, 2, 2, 1, 0, 1) X(0, 2, 2, 2, 1, 1, 0) X(0, 2, 2, 2, 1, 1, 1) X(0, 2, 2, 2, 2, 0, 1) \
    X(0, 2, 2, 2, 2, 1, 0) X(0, 2, 2, 2, 2, 1, 1) X(0, 2, 2, 4, 1, 1, 1) X(0, 2, 2, 4, 2, 0, 1) X(0, 2, 3, 2, 1, 0, 1) \
    X(0, 2, 3, 2, 1, 1, 1) X(0, 2, 3, 2, 2, 1, 1) X(0, 2, 3, 4, 2, 0, 1) X(0, 4, 2, 2, 1, 0, 1) X(0, 4, 2, 2, 1, 1, 0) \
    X(0, 4, 2, 2, 1, 1, 1) X(0, 4, 2, 2, 2, 0, 1) X(0, 4, 2, 2, 2, 1, 0) X(0, 4, 2, 2, 2, 1, 1) X(0, 4, 2, 4, 1, 1, 1) \
    X(0, 4, 2, 4, 2, 0, 1) X(0, 4, 3, 2, 1, 0, 1) X(0, 4, 3, 2, 1, 1, 1) X(0, 4, 3, 2, 2, 1, 1) X(0, 4, 3, 4, 2, 0, 1) \
    X(0, 8, 2, 2, 1, 1, 1) X(0, 8, 2, 2, 2, 1, 1) X(0, 8, 3, 2, 1, 1, 1) X(0, 8, 3, 2, 2, 1, 1) X(1, 1, 2, 2, 1, 0, 1) \
    X(1, 1, 2, 2, 1, 1, 1) X(1, 1, 2, 2, 2, 0, 1) X(1, 1, 2, 2, 2, 1, 1) X(1, 2, 2, 2, 1, 0, 1) X(1, 2, 2, 2, 1, 1, 1) \
    X(1, 2, 2, 2, 2, 0, 1) X(1, 2, 2, 2, 2, 1, 1) X(1, 2, 3, 2, 1, 1, 1) X(1, 2, 3, 2, 2, 1, 1) X(1, 4, 2, 2, 1, 0, 1) \
    X(1, 4, 2, 2, 1, 1, 1) X(1, 4, 2, 2, 2, 0, 1) X(1, 4, 2, 2, 2, 1, 1) X(1, 4, 3, 2, 1, 1, 1) X(1, 4, 3, 2, 2, 1, 1) \
    X(1, 8, 2, 2, 1, 1, 1) X(1, 8, 2, 2, 2, 1, 1) X(1, 8, 3, 2, 1, 1, 1)

// forward, row-scaled f16 storage: X(NG, DEPTH, RT, KB, AS, EX): k_mf_forward_b16_lds<NG, DEPTH, RT, KB, f16s_t, AS, EX>.
// Only the keys the planner returns with no knob set (the bf16-storage defaults at 16 / 32 / 64 / 128 frames): (a).
#define MF_FWD_S16_VARIANTS(X) X(1, 3, 2, 2, 0, 0) X(2, 3, 2, 2, 1, 0) X(4, 3, 4, 2, 0, 0) X(8, 3, 2, 2, 1, 0)

// back-projection, fp32 MFMA: k_mf_backproject<NG, DEPTH, VT>
#define MF_BWD_F32_VARIANTS(X) \
    X(1, 1, 1) X(1, 1, 2) X(1, 2, 1) X(1, 2, 2) X(1, 3, 1) X(1, 3, 2) \
    X(2, 1, 1) X(2, 1, 2) X(2, 2, 1) X(2, 2, 2) X(2, 3, 1) X(2, 3, 2) \
    X(4, 1, 1) X(4, 1, 2) X(4, 2, 1) X(4, 2, 2) X(4, 3, 1) X(4, 3, 2)

// back-projection, bf16 storage: X(LDS, NG, DEPTH, VT, EW). LDS 0: k_mf_backproject_b16<NG, DEPTH, VT>;
// LDS 1: k_mf_backproject_b16_lds<NG, DEPTH, VT, bf16_t, EW>
#define MF_BWD_B16_VARIANTS(X) \
    X(0, 1, 3, 1, 0) X(0, 1, 3, 2, 0) X(0, 2, 3, 1, 0) X(0, 2, 3, 2, 0) X(0, 4, 3, 1, 0) X(0, 4, 3, 2, 0) \
    X(1, 1, 1, 1, 1) X(1, 1, 1, 2, 1) X(1, 1, 2, 1, 1) X(1, 1, 2, 2, 1) X(1, 1, 3, 1, 0) X(1, 1, 3, 1, 1) \
    X(1, 1, 3, 2, 0) X(1, 1, 3, 2, 1) X(1, 2, 1, 1, 1) X(1, 2, 1, 2, 1) X(1, 2, 2, 1, 1) X(1, 2, 2, 2, 1) \
    X(1, 2, 3, 1, 0) X(1, 2, 3, 1, 1) X(1, 2, 3, 2, 0) X(1, 2, 3, 2, 1) X(1, 4, 1, 1, 1) X(1, 4, 1, 2, 1) \
    X(1, 4, 2, 1, 1) X(1, 4, 2, 2, 1) X(1, 4, 3, 1, 0) X(1, 4, 3, 1, 1) X(1, 4, 3, 2, 0) X(1, 4, 3, 2, 1) \
    X(1, 8, 2, 1, 1) X(1, 8, 3, 1, 1)

// back-projection, split-A on bf16 pieces: k_mf_backproject_b16_lds<NG, DEPTH, VT, float, EW>
#define MF_BWD_X3_VARIANTS(X) \
    X(1, 2, 1, 0) X(1, 2, 1, 1) X(1, 2, 2, 0) X(1, 3, 1, 0) X(1, 3, 2, 0) X(2, 2, 1, 0) \
    X(2, 2, 1, 1) X(2, 2, 2, 0) X(2, 3, 1, 0) X(2, 3, 2, 0) X(4, 2, 1, 0) X(4, 2, 1, 1) \
    X(4, 2, 2, 0) X(4, 3, 1, 0) X(4, 3, 2, 0)

// back-projection, row-scaled f16 storage: X(NG, DEPTH, VT, EW): k_mf_backproject_b16_lds<NG, DEPTH, VT, f16s_t, EW>.
// The planner's defaults only: VT 2 (ld % 128 == 0) or 1 at 16 / 32 / 64 frames, VT 1 at 128; W loaded early.
#define MF_BWD_S16_VARIANTS(X) \
    X(1, 3, 1, 1) X(1, 3, 2, 1) X(2, 3, 1, 1) X(2, 3, 2, 1) X(4, 3, 1, 1) X(4, 3, 2, 1) X(8, 3, 1, 1)

// back-projection, split-A on f16 pairs: k_mf_backproject_h16<NG, DEPTH, EW, MW>
#define MF_BWD_H16_VARIANTS(X) \
    X(1, 2, 0, 1) X(1, 2, 0, 2) X(1, 2, 1, 1) X(1, 2, 1, 2) X(1, 3, 0, 2) X(2, 2, 0, 1) \
    X(2, 2, 0, 2) X(2, 2, 1, 1) X(2, 2, 1, 2) X(2, 3, 0, 2) X(4, 2, 0, 1) X(4, 2, 0, 2) \
    X(4, 2, 1, 1) X(4, 2, 1, 2) X(4, 3, 0, 2) X(8, 2, 0, 1) X(8, 2, 1, 1) X(8, 3, 0, 1)
