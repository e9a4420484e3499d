// One time step of a recurrence whose input projection is hoisted (prenet bi-GRU, encoder LSTM): the statements shared by
// seq_step_kernel and seq_step_save_kernel of scan.hip (the latter serves context_grad.hip), so that both give the same bits.
// Weights in fragment order (scan.hip, build_wfrag_kernel), one 16-row x 16-utterance MFMA tile per workgroup, K over 4 waves.
#pragma once
#include "common.h"
#include "ar_shared.h"
#include <math.h>

struct SeqP {
    const float *Wf;      // [dir][H/4 row groups][4 waves][SW][64] float4
    const float *b_hh;    // GRU: [dir][3H]; LSTM: unused (folded into Gi)
    const float *Gi;      // [B*T][ndir*G*H]  input projection (+ biases)
    float *hbuf;          // [2][ndir][nbt][H*16]
    float *cbuf;          // LSTM cell state [ndir][nbt][H*16]
    float *out;           // [B][T][ndir*H]
    const int *len;       // valid steps per utterance (nbt*16) or null = T for b < B
    const int *row0;      // first row of every utterance in Gi / out (ragged rows) or null = b * T
    int H, nbt, B, T, ndir;
};

// What the backward of the LSTM reads again (context_grad.hip), by output row: the activated gates i | f | g | o, the cell state
// and its tanh.
struct SeqSave {
    float *gates;         // [rows][4H]
    float *cell;          // [rows][H]
    float *tanhc;         // [rows][H]
};

template <int G, int SW, bool SAVE>   // G = 3 GRU, 4 LSTM; SAVE (LSTM only): also store `sv`
__device__ __forceinline__ void seq_step_body(const SeqP &p, int step, const SeqSave &sv) {
    __shared__ float red[4][16][17];
    __shared__ float gate[16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = blockIdx.x, dir = blockIdx.y, H = p.H;
    const size_t hsz = (size_t)p.nbt * H * 16;
    const float *hin = p.hbuf + ((size_t)(step & 1) * p.ndir + dir) * hsz;
    float *hout = p.hbuf + ((size_t)((step + 1) & 1) * p.ndir + dir) * hsz;
    const int bt = blockIdx.z;                     // one utterance tile per workgroup
    // cell-update operands of wave 0's lanes are requested first: they do not depend on this step's
    // W_hh h, so their latency hides under the fragment loads and the MFMAs
    const int u = (tid >> 4) & 3, b = tid & 15, bg = bt * 16 + b, unit = 4 * rg + u;
    bool act = false;
    int tpos = 0;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, bh0 = 0.f, bh1 = 0.f, bh2 = 0.f, hold = 0.f, cold = 0.f;
    const size_t hi = hl_index(H, bg, unit);
    if (tid < 64) {
        const int L = p.len ? p.len[bg] : (bg < p.B ? p.T : 0);
        if (step < L) {
            act = true;
            tpos = dir == 0 ? step : L - 1 - step;
            const float *gi = p.Gi + ((p.row0 ? (size_t)p.row0[bg] : (size_t)bg * p.T) + tpos) * (p.ndir * G * H) + (size_t)dir * G * H + unit;
            g0 = gi[0]; g1 = gi[H]; g2 = gi[2 * H];
            if (G == 3) {
                const float *bh = p.b_hh + (size_t)dir * 3 * H + unit;
                bh0 = bh[0]; bh1 = bh[H]; bh2 = bh[2 * H];
                hold = hin[hi];
            } else {
                g3 = gi[3 * H];
                cold = p.cbuf[(size_t)dir * hsz + hi];
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    float4 wf[SW];
    load_wfrag<SW>(p.Wf + (size_t)dir * (H / 4) * (H / 16) * 64 * 4, rg, 4, wave, lane, wf);
    const f32x4 acc = mv16<SW>(wf, hin, H, bt, wave, lane);
    const float v = reduce4(red, acc, wave, lane, tid);
    gate[tid >> 4][tid & 15] = v;
    __syncthreads();
    if (act) {
        float hn;
        if (G == 3) {
            const float r = sigmoidf_(g0 + (gate[u][b] + bh0));
            const float z = sigmoidf_(g1 + (gate[4 + u][b] + bh1));
            const float n = tanhf(g2 + r * (gate[8 + u][b] + bh2));
            hn = (1.0f - z) * n + z * hold;
        } else {
            const float ig = sigmoidf_(g0 + gate[u][b]), fg = sigmoidf_(g1 + gate[4 + u][b]);
            const float gg = tanhf(g2 + gate[8 + u][b]), og = sigmoidf_(g3 + gate[12 + u][b]);
            const float cn = fg * cold + ig * gg;
            p.cbuf[(size_t)dir * hsz + hi] = cn;
            const float tc = tanhf(cn);
            hn = og * tc;
            if (SAVE) {                            // ndir == 1, rows b * T + t
                const size_t row = (size_t)bg * p.T + tpos;
                float *gs = sv.gates + row * (4 * H) + unit;
                gs[0] = ig; gs[H] = fg; gs[2 * H] = gg; gs[3 * H] = og;
                sv.cell[row * H + unit] = cn;
                sv.tanhc[row * H + unit] = tc;
            }
        }
        hout[hi] = hn;
        p.out[((p.row0 ? (size_t)p.row0[bg] : (size_t)bg * p.T) + tpos) * (p.ndir * H) + (size_t)dir * H + unit] = hn;
    }
}
