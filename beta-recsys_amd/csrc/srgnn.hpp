// SR-GNN (csrc/srgnn.hip): the limits of the model and the tile sizes its launches are cut by.
// tests/srgnn_edges.py restates them (its fixtures sit one under, at and one over each) and
// tests/test_srgnn_host.py reads this file to hold the two together.
#pragma once

namespace hiprec {

constexpr int kSrgnnMaxHidden = 128;      // `hidden_size`: two values per lane of one wave
constexpr int kSrgnnMaxStep = 4;          // repetitions of the gated cell
constexpr int kSrgnnMaxLen = 256;         // T: one builder thread per position
constexpr int kSrgnnMaxBatch = 1024;      // B: sessions of a step

constexpr int kSrgnnRowTile = 64;         // rows of one grouped-GEMM block (kTM of csrc/ncf.hip)
constexpr int kSrgnnSlabRows = 128;       // rows of one partial of the fixed-order column sums (kColsumRows of csrc/ncf.hip)
constexpr int kSrgnnWaves = 4;            // sessions / nodes of one workgroup of the wave-per-row kernels
constexpr int kSrgnnKSlices = 16;         // fixed-order K slices of d a = dscores E[1:] (kMaxGroup of csrc/gemm.hpp)

}  // namespace hiprec
