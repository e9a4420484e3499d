// Vocoder scoring head (nll.hip): what vocoder_host.hip hands it after every chunk of the teacher-forced scan.
#pragma once
#include "common.h"

constexpr int NLL_HF = 256, NLL_CLS = 256;    // the head is built for the reference's size_h_fc and 8-bit mu-law (config.py:69,77)

struct NllPart { double sum; int n, ok; };    // one (utterance, workgroup) record: nll sum, scored samples, correct ones

struct NllHead {
    const float *hall;                   // [B][CH][Hr] h_t of the chunk (rows past an utterance's scored length are stale)
    const float *w1, *b1, *w2, *b2;      // fc1 (256, Hr), fc2 (256, 256): plain row-major
    const int64_t *audio;                // (B, L) mu-law classes: step t reads audio[b, t], its target is audio[b, t + 1]
    const int *slen;                     // [B] DEVICE scored steps per utterance (<= L - 1)
    float *nll;                          // (B, L - 1) or null
    NllPart *part;                       // [B][tiles] records of this chunk
    unsigned *status; unsigned status_tag;
    int B, L, CH, t0, Hr;                // t0 = first step of the chunk
};

int vq_tf_nll_prepare();                 // once per handle: the head kernel's dynamic-LDS attribute
int vq_tf_nll_tiles(int CH);             // records per utterance and chunk
// Scores the chunk and adds its records onto nll_sum / n_scored / n_correct (DEVICE, zeroed by the caller before the first chunk).
int vq_tf_nll_chunk(const NllHead &p, double *nll_sum, int64_t *n_scored, int64_t *n_correct, hipStream_t s);
