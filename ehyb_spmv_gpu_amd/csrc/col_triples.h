// The column words of the window kernel as the DEVICE holds them (cfg.ell_triples).  The host layout stores two 16-bit window
// columns per value pair and group (ehyb.h: EHYB_ARR_ELL_COL) and stays the definition; ehyb_plan_upload sends this form instead.
//
// The rows of a node with three unknowns list their columns in node triples c, c+1, c+2 with one mirror flag, so a slab whose
// every group is such a list stores one 16-bit BASE per triple: a third of the words, and two column loads per six value pairs.
//
// A slab is triple-coded only if all of these hold:
//   - it has no inline residual pairs and is not a relative slab;
//   - its window has at least 3 slots (a padding triple decodes to columns 0, 1, 2);
//   - for every group the 2 np 16-bit entries (np = the slab's pairs), cut into threes from the front, are triples (b, b+1, b+2)
//     with bit 15 equal in all three, or (0, 0, 0) (padding); a remainder of two entries is (b, b+1) or (0, 0).
// It then holds T = ceil(2 np / 3) bases per group, two per 32-bit word (low half first): W = ceil(T / 2) words per group at
// [word][group] with stride G, as the pair form.  A base carries bit 15 as the mirror flag of its triple; a padding triple is
// base 0.  With (A, B) = word j: pair 3j reads columns (A, A+1), pair 3j+1 (A+2, B), pair 3j+2 (B+1, B+2).
// Every other slab is copied unchanged, and so is every slab of a plan with symmetric pairs, an inline residual and a window
// small enough for four columns per pass (ehyb_spmm_max_k = 4): the kernel of that one combination does not decode the form.
// In the device slab records word SLAB_COL_PTR is the slab's offset in the transcoded array and bit 6 of word SLAB_SHAPE
// (kSlabTriples) marks a triple-coded slab; nothing else changes.
// No HIP in here: the transcoder builds and runs on the CPU.
#pragma once
#include "ehyb_internal.h"

namespace ehyb {

constexpr uint32_t kSlabTriples = 0x40u;  // bit 6 of a DEVICE slab record's shape word (free in pack_slab_shape)

// Words per group of a triple-coded slab of np pairs
inline uint32_t triple_words(uint32_t np) { return ((2 * np + 2) / 3 + 1) / 2; }

// The device copies of H.ell_col and H.slab_meta.  triples = false: the host arrays as they are.  Returns the number of words.
// words / meta may be null (count only).  Deterministic: the same arrays whatever the number of host threads.
int64_t device_cols(const HostLayout& H, bool triples, BigVec<uint32_t>* words, std::vector<uint32_t>* meta);

}  // namespace ehyb
