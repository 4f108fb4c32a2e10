// GRU4Rec (csrc/gru4rec.hip): the limits of the model and the tile sizes its launches are cut by.
// tests/gru4rec_edges.py restates them (its fixtures sit one under, at and one over each) and
// tests/test_gru4rec_host.py reads this file to hold the two together.
#pragma once

namespace hiprec {

constexpr int kGru4recMaxLayers = 3;
constexpr int kGru4recMaxHidden = 128;    // every entry of `layers`
constexpr int kGru4recMaxDim = 128;       // `embedding` (unconstrained input)
constexpr int kGru4recMaxBatch = 2048;    // B: slots of a step
constexpr int kGru4recMaxSample = 4096;   // S: extra sampled items of a step

constexpr int kGru4recRowTile = 64;       // batch rows of one grouped-GEMM block (kTM of csrc/ncf.hip)
constexpr int kGru4recCandTile = 64;      // candidate columns of one grouped-GEMM block (kTN of csrc/ncf.hip)
constexpr int kGru4recSlabRows = 128;     // rows of one partial of the fixed-order column sums (kColsumRows of csrc/ncf.hip)
constexpr int kGru4recLossWaves = 4;      // rows of the score block that one loss workgroup owns (one wave each)

}  // namespace hiprec
