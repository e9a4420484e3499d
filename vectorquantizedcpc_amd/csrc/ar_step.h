// The launch-per-step sample loop (vocoder.hip) -- interface towards the host side (vocoder_host.hip, vocoder_stream.hip).
#pragma once
#include "common.h"
#include "ar_xcd.h"

// ------------------------------------------------------------------------------------------
// Autoregressive sample loop.  Per sample t, three launches (each an all-gather boundary):
//   ar_gru : x_{t-1} = argmax of the fc2 candidates; h_t = GRUCell(Gemb[x_{t-1}] + Gcond, h_{t-1})
//   ar_fc1 : a_t = relu(W1 h_t + b1)
//   ar_fc2 : l_t = W2 a_t + b2; per 16-class row group the Gumbel-max candidate (score, class)
// The categorical draw is an exponential race (argmax_k l_k + g_k, the algorithm of ATen's
// Categorical.sample), which decomposes over class subsets: fc2 is spread over 16 CUs and the
// 16 candidates per utterance are merged by the next step's GRU kernel.
// Per-call quantities live in a device-side ArCall so one captured graph serves every call.
// ------------------------------------------------------------------------------------------
// Continuous batching: a decode SLOT (one MFMA column) runs utterances back to back.  Utterances
// start at replay boundaries, so per (replay, slot) there is at most one XdSeg: row = its index in this
// call's inputs/outputs (-1 = idle), t0 = global step of its sample 0, len = its samples,
// utt = its sampling-stream id.

struct ArCall {
    const float *Gcond;        // [sum of the utterances' frames][3Hr] = W_ih[:, de:] cond + b_ih, ragged: utterance `row` starts at row gbase[row]
    const int *gbase;          // [B] first Gcond row of every utterance (prefix sums of the conditioning frame counts)
    const int64_t *inputs;     // teacher forcing (B, Ts) or null
    float *wav;                // (B, Lout) or null
    int64_t *mulaw;            // (B, Lout) or null
    float *logits;             // (B, Ts, n_cls) or null
    const XdSeg *slots;        // [replays][Sp] what every decode slot is doing during each graph replay
    int S, Sp;                 // steps per replay (t_base is a multiple of it), slots (multiple of 16)
    int n_rep;                 // rows of `slots`
    int F, Ts, Lout, max_t, nbt;
    unsigned long long seed;
    int t_base;                // advanced on device after every graph replay
    // teacher-forced scan (Vocoder.forward): only the GRU step runs per sample; h_t of every step of the current
    // chunk is kept, row-major, for the two batched GEMMs (fc1 + ReLU, fc2) that follow the chunk
    float *hall;               // [B][CH][Hr] or null
    int CH, hall_t0;           // chunk length (a multiple of S); first step of the chunk in flight (advanced on device)
    // A chunk of a stream (vqcpc_vocoder_stream_next).  Every utterance resumes at absolute sample s0: its slot rows carry
    // t0 - s0 and s0 + len, so the step kernels see absolute sample indices (Philox counter, conditioning frame) unchanged, and
    // wav / mulaw point s0 - 1 columns in front of a buffer whose column 0 takes sample s0 - 1 again.  ar_next_row_kernel
    // seeds a resumed slot (h_in in its state column, x_in as every candidate of its first step) and copies a finished one's
    // final state to h_out.  All null / 0 for a one-shot call.
    const float *h_in;         // [B][Hr] or null: fresh start (s0 == 0)
    const int *x_in;           // [B]
    float *h_out;              // [B][Hr] or null
    int s0;
    // A scoring call (vqcpc_vocoder_nll): every utterance starts at step 0 in its own slot, so `slots` holds ONE row for all replays
    // and a slot goes idle (row -1, what the full table says) once its utterance's steps are done: the table does not grow with
    // the length of the call.  0 for every other call.
    int one_row;
};

struct ArModel {               // constant per handle (baked into the captured graph)
    // Cell-update operands in "unit quads": for row group rg (4 hidden units) and unit u, ONE float4 = (r, z, n, 0).
    // A gate wave's lane then needs one 16-byte load per table instead of three 4-byte loads H apart, and the 16
    // slots of a tile read 1 KiB contiguous (gcur4) -- the [3H] layouts cost a whole 128-B line per 16 bytes used.
    const float4 *bh4;         // [Hr/4][4]            b_hh
    const float4 *Gemb4;       // [n_cls][Hr/4][4]     emb . W_ih[:, :de]^T
    const float *Gemb;         // [n_cls][3Hr] (unused by the step kernels; kept for tools)
    const float *Wf_hh12;      // W_hh in packed 12-row groups (ar_gru_kernel: no padding rows streamed)
    const float *Wf_hh16;      // W_hh in gate-major 16-row tiles (large-batch kernel: no padding rows)
    float4 *gcur4;             // [Hr/4][Sp][4] the Gcond row every slot uses during the replay in flight (gc_replay), unit quads
    int gc_replay;             // 1: upsample % steps_per_graph == 0, so a slot stays on one conditioning frame per replay
    int live_last;             // decode slots in use in the last tile (1..16): lanes of dead columns re-read column 0
    int lead6;                 // ar_gru_kernel requests fragments 6 super-steps ahead instead of 3 (see there)
    const float *Wf_fc1, *b_fc1, *Wf_fc2, *b_fc2, *mulaw_tab;
    const float *Wf_fc1h;      // fc1 in 8-row groups (few tiles in flight: twice the workgroups, half the weight bytes each)
    float *hbuf;               // [2][nbt][Hr*16]
    float *a1;                 // [nbt][Hf*16]
    float *cand_s;             // [Bpad][n_cls / 16] best score of each 16-class row group
    int *cand_k;               // [Bpad][n_cls / 16] its class
    XdSeg *cur;                // [Sp] the slot row of the replay in flight (copied from ArCall::slots between
                               // replays): a fixed address, so the step kernels read it without first waiting for ArCall
    // fused fc2 || GRU launch: candidates as 8-byte granules {(tag << 10 | class), score}, tag = step + 1, one 128-B
    // line per producing workgroup: [tile][16 row groups][16 slots]
    unsigned long long *candg;
    unsigned *abort_dev;       // set when a candidate wait timed out: later steps stop waiting
    unsigned *abort_host;      // the same, host-mapped: the next call on the handle reports it
    unsigned timeout_ticks;    // bound of the in-kernel candidate waits (100 MHz ticks)
    int dbg_drop_t;            // tests: the fc2 team of row group 3, tile 0 skips its candidate publish at this step (-1: never)
    int fused;                 // 0: three launches per sample; 1: fc2 + draw ride in the GRU launch (candidates in candg)
    int Hr, Hf, n_cls, upsample;
};

#define CAND_TAG_BITS 22       // a fused launch tags its candidate granules with the step, modulo 2^22

// What the launchers need to know of the handle.
// big_min_tiles: utterance tiles from which the LDS-staged GRU kernel is used (0 = never); *big_attr_set: that kernel's
// dynamic-LDS attribute has been set (launch_ar_steps sets it once).
struct ArStep { int Hr, Hf, n_cls, big_min_tiles; bool *big_attr_set; };

int build_wfrag12(const float *W, int ldw, int n_rg, int K, int H, DevBuf &out, hipStream_t s = 0);     // reserves `out`
bool use_big(const ArStep &a, int nbt);
// One GRU-step launch for local step `tl`; nf = fc2 blocks of the previous step in front (fused launch, 0 = none).
int launch_gru_step(const ArStep &a, const ArModel &m, const ArCall *call, int tl, int nbt, int nf, hipStream_t s);
int launch_fc1_step(const ArStep &a, const ArModel &m, const ArCall *call, int tl, int nbt, hipStream_t s);
void launch_fc2_step(const ArStep &a, const ArModel &m, const ArCall *call, int tl, int nbt, hipStream_t s);   // plain candidate arrays
// The slot row (and Gcond rows) of the replay that starts at the call's t_base: before replay 0; launch_ar_steps ends with it.
void launch_next_row(const ArModel &m, const ArCall *call, int nbt, hipStream_t s);
// n steps of one replay.  tf: teacher-forced scan -- x_{t-1} comes from the inputs, so only the GRU step runs per sample.
int launch_ar_steps(const ArStep &a, const ArModel &m, ArCall *call, int nbt, int n, bool tf, hipStream_t s);
