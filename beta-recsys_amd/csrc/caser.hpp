// Caser (csrc/caser.hip): the limits of the model and the tile sizes of its kernels.  tests/caser_edges.py restates
// them (its fixtures sit one under, at and one over each tile) and tests/test_caser_host.py reads this file to hold
// the two together.
#pragma once

namespace hiprec {

constexpr int kCaserMaxDim = 128;      // d
constexpr int kCaserMaxLen = 10;       // L
constexpr int kCaserMaxNv = 16;        // n_v
constexpr int kCaserMaxNh = 64;        // n_h
constexpr int kCaserMaxT = 16;         // T
constexpr int kCaserMaxN = 64;         // N

constexpr int kCaserSeqTile = 8;       // sequences of one convolution-forward workgroup (8 x L <= 80 rows = 5 MFMA row tiles)
constexpr int kCaserSlabRows = 64;     // the fixed-order folds of d conv_h / d conv_v: at least this many rows per partial ...
constexpr int kCaserMaxSlabs = 16;     // ... and at most this many partials (rows per partial = ceil(B / partials))
constexpr int kCaserChunk = 256;       // rows of a partial that the d conv_h kernel stages in LDS at a time

}  // namespace hiprec
