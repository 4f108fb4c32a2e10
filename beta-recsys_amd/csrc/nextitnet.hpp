// NextItNet (csrc/nextitnet.hip): the limits of the model and the tile sizes of its kernels.  D and T are bounded by
// kSeqMaxDim / kSeqMaxLen of csrc/seqrec.hpp.
#pragma once

namespace hiprec {

constexpr int kNinMaxKernel = 4;       // kernel_size
constexpr int kNinMaxBlocks = 16;      // residual blocks R = len(dilations) * block_num

constexpr int kNinTimeTile = 32;       // time positions of one sequence a convolution workgroup owns (2 MFMA row tiles)
constexpr int kNinColChunk = 32;       // output columns of the weight slab staged in LDS at a time (2 MFMA column tiles)
constexpr int kNinWgradRows = 32;      // rows m = b T + t of one weight-gradient row tile
constexpr int kNinMaxSlabs = 32;       // at most this many partials of a weight gradient; slab q walks tiles q, q + slabs, ...

constexpr int kNinCeRows = 32;         // cross-entropy tile: labelled rows ...
constexpr int kNinCeItems = 64;        // ... x items
constexpr int kNinCeMaxSplits = 16;    // catalogue splits of the row-side kernels, folded in split order
constexpr int kNinCeTargetBlocks = 1024;

}  // namespace hiprec
