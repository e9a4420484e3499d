// Negative-sampling protocol of CPC scoring (project spec; restated in vectorquantizedcpc_amd/synth.py, cpc_negatives).
//
// The reference draws its negatives from torch's global CPU generator (model.py:251-268), a stream no device kernel can
// share.  The algorithm is kept, the stream is fixed here: for prediction step k (1-based) draw i of that step is
//
//     w = Philox4x32-10(counter = (i >> 2, (which << 16) | k, stream_id, 0), key = (seed & 0xffffffff, seed >> 32))[i & 3]
//
//   which = 0: utterance draws, i = flat index into (Utt, Neg),           u = w mod Utt
//   which = 1: position draws,  i = flat index into (Spk, Utt, Neg, L),   r = 1 + w mod (L - 1),  s = (r + t) mod L
//
// (u, s) are the two index arrays of model.py:282, s after the remainder of model.py:272: negative j of anchor
// (spk, utt, t) at step k is the row z[spk * Utt + u[utt, j], s[spk, utt, j, t] + k].  `mod` as torch.randint reduces its
// words; the bias is below 2^-24 at these ranges.  philox_word of ar_shared.h is the one Philox of the library.
#pragma once
#include "ar_shared.h"

constexpr unsigned CPC_WHICH_UTT = 0u, CPC_WHICH_SEQ = 1u;

__device__ __forceinline__ unsigned cpc_word(unsigned which, int k, unsigned i, unsigned stream_id, unsigned k0, unsigned k1) {
    return philox_word(i >> 2, (which << 16) | (unsigned)k, stream_id, k0, k1, (int)(i & 3u));
}
__device__ __forceinline__ int cpc_draw_utt(int k, unsigned i, int Utt, unsigned stream_id, unsigned k0, unsigned k1) {
    return (int)(cpc_word(CPC_WHICH_UTT, k, i, stream_id, k0, k1) % (unsigned)Utt);
}
__device__ __forceinline__ int cpc_draw_seq(int k, unsigned i, int t, int L, unsigned stream_id, unsigned k0, unsigned k1) {
    const int r = 1 + (int)(cpc_word(CPC_WHICH_SEQ, k, i, stream_id, k0, k1) % (unsigned)(L - 1));
    return (r + t) % L;
}
