// vocoder_stream.hip -- vqcpc_vocoder_stream_*: chunked decode on the vocoder handle of vocoder_host.hip.
#include "vocoder_internal.h"

// ------------------------------------------------------------------------------------------
// streaming decode (vqcpc_vocoder_stream_*): the prenet runs once at open over every utterance's full length (it is
// bidirectional); each chunk is then one call of the decode loop whose utterances RESUME -- at absolute sample pos, from the h
// and x the previous chunk left -- so the chunks concatenate to exactly what one generate() call gives (same Philox counters,
// same conditioning frames, same state).  Chunks plan with xcm = 0: up to xcm_max utterances run on the per-XCD decoders of
// ar_xcd.hip (more than 32 back to back in their slots, each one a resumed segment), beyond that on the launch path.
// ------------------------------------------------------------------------------------------
struct vqcpc_vocoder_stream {
    vqcpc_vocoder *v = nullptr;
    int B = 0, Tc = 0;
    unsigned long long seed = 0;
    UttLayout lay;                       // per utterance: frames and samples in all, sampling-stream id, first conditioning row
    DevBuf cond, gcond, gbase_dev;       // the stream's own prenet output [grows][2Hp] and conditioning rows (W_ih[:, de:] cond + b_ih) [grows][3Hr]
    DevBuf h, x;                         // [2][B][Hr] fp32, [2][B] int: chunk c resumes from half c & 1 and leaves half (c + 1) & 1
    DevBuf owav, omul;                   // (B, n + 1) decode buffers of the chunk in flight
    int64_t pos = 0, total = 0, last_pos = 0;
    int last_n = 0, chunks = 0;
};

// (B, n + 1) decode buffers -> the caller's (B, n) outputs; the row's last class is the next chunk's x_in
__global__ void stream_out_kernel(const float *__restrict__ owav, const int64_t *__restrict__ omul, int B, int n, float *wav,
                                  int64_t *mulaw, int *x_next) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * n) return;
    const size_t b = i / n, j = i % n, src = b * (n + 1) + 1 + j;
    wav[i] = owav[src];
    if (mulaw) mulaw[i] = omul[src];
    if (j == (size_t)n - 1) x_next[b] = (int)omul[src];
}

static int stream_chunk(vqcpc_vocoder_stream *st, int64_t pos, int n, int ci, float *wav, int64_t *mulaw, hipStream_t s) {
    vqcpc_vocoder *v = st->v;
    const auto &d = v->d;
    const int B = st->B, Hr = d.Hr;
    const int *samples = st->lay.lens.data() + (B + 15) / 16 * 16;
    // samples of every utterance in [pos, pos + n); the resident decoders take one priming step in front of them
    std::vector<int> nr(B), res(B);
    for (int b = 0; b < B; ++b) {
        const int64_t left = samples[b] - pos;
        nr[b] = left <= 0 ? 0 : (left < n ? (int)left : n);
        res[b] = nr[b] > 0 ? nr[b] + 1 : 0;
    }
    CallPlan cp;
    static_cast<UttLayout &>(cp) = st->lay;
    PlanOpts po = plan_opts(v);          // never the matrix-core decoders: ar_xcd.hip up to xcm_max utterances in flight
    po.xcm = 0; po.xcm_min = po.xcm_max;
    VQ_REQUIRE(plan_decode(po, res.data(), cp.utt.data(), longest_first(res.data(), B), cp.dp), "vocoder stream: a decode slot's "
               "schedule does not fit the resident decoders; use more slots or xcd = -1");
    if (cp.dp.path == 0) TRY(plan_launch_tables(po, nr.data(), longest_first(nr.data(), B), false, B, (int)pos, cp));
    TRY(begin_call(v, cp, B));
    const size_t ob = (size_t)B * (n + 1);
    TRY(st->owav.reserve(ob * sizeof(float)));
    TRY(st->omul.reserve(ob * sizeof(int64_t)));
    HIP_TRY(hipMemsetAsync(st->owav.p, 0, ob * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(st->omul.p, 0, ob * sizeof(int64_t), s));
    const int in = ci & 1, out = (ci + 1) & 1;
    const Resume rs{XdResume{(int)pos, ci > 0 ? st->h.as<float>() + (size_t)in * B * Hr : nullptr, ci > 0 ? st->x.as<int>() + (size_t)in * B : nullptr,
                             st->h.as<float>() + (size_t)out * B * Hr},
                    n + 1, st->gcond.as<float>(), st->gbase_dev.as<int>()};
    if (v->last_path != 0) v->last_path = 1;      // a chunk that fails from here on ran no decode loop
    if (cp.dp.path != 0) TRY(run_resident(v, cp, 2 * st->Tc, st->seed, st->owav.as<float>(), st->omul.as<int64_t>(), s, &rs));
    else TRY(run_launch_path(v, cp, nullptr, 2 * st->Tc, 0, st->seed, st->owav.as<float>(), st->omul.as<int64_t>(), nullptr, s, &rs));
    hipLaunchKernelGGL(stream_out_kernel, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, s, st->owav.as<float>(),
                       st->omul.as<int64_t>(), B, n, wav, mulaw, st->x.as<int>() + (size_t)out * B);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_stream_open(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                                         const int *n_codes, uint64_t seed, uint32_t utt_base, const uint32_t *utt_ids,
                                         vqcpc_vocoder_stream **out, void *stream) {
    VQ_REQUIRE(v && idx && speaker && out, "vqcpc_vocoder_stream_open: null argument");
    VQ_REQUIRE(B > 0 && Tc > 0, "vocoder stream: need B > 0 and Tc > 0 (got %d, %d)", B, Tc);
    *out = nullptr;
    const auto &d = v->d;
    hipStream_t s = (hipStream_t)stream;
    vqcpc_vocoder_stream *st = new vqcpc_vocoder_stream();
    st->v = v; st->B = B; st->Tc = Tc; st->seed = seed;
    st->total = (int64_t)2 * d.upsample_t * Tc;
    CallPlan cp;                         // the layout only: nothing is decoded at open
    int rc = utt_layout(B, Tc, n_codes, d.upsample_t, utt_base, utt_ids, cp);
    st->lay = cp;
    if (rc == VQCPC_OK) rc = begin_call(v, cp, B);
    if (rc == VQCPC_OK) rc = run_conditioning(v, st->lay, idx, speaker, B, Tc, st->cond, st->gcond, st->gbase_dev, s);
    if (rc == VQCPC_OK) rc = st->h.reserve((size_t)2 * B * d.Hr * sizeof(float));
    if (rc == VQCPC_OK) rc = st->x.reserve((size_t)2 * B * sizeof(int));
    if (rc != VQCPC_OK) { vqcpc_vocoder_stream_close(st); return rc; }
    *out = st;
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_stream_next(vqcpc_vocoder_stream *st, int n_samples, float *wav, int64_t *mulaw, void *stream) {
    VQ_REQUIRE(st && wav, "vqcpc_vocoder_stream_next: null argument");
    const int up = st->v->d.upsample_t;
    VQ_REQUIRE(n_samples > 0 && n_samples % up == 0, "vocoder stream: n_samples = %d must be a positive multiple of %d", n_samples, up);
    VQ_REQUIRE(st->pos < st->total, "vocoder stream: all %lld samples have been decoded", (long long)st->total);
    TRY(stream_chunk(st, st->pos, n_samples, st->chunks, wav, mulaw, (hipStream_t)stream));
    st->last_pos = st->pos; st->last_n = n_samples;
    st->chunks += 1;
    st->pos = st->pos + n_samples < st->total ? st->pos + n_samples : st->total;
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_stream_redo(vqcpc_vocoder_stream *st, float *wav, int64_t *mulaw, void *stream) {
    VQ_REQUIRE(st && wav, "vqcpc_vocoder_stream_redo: null argument");
    VQ_REQUIRE(st->chunks > 0, "vocoder stream: no chunk to repeat");
    return stream_chunk(st, st->last_pos, st->last_n, st->chunks - 1, wav, mulaw, (hipStream_t)stream);
}

extern "C" int vqcpc_vocoder_stream_position(const vqcpc_vocoder_stream *st, int64_t *done, int64_t *total) {
    VQ_REQUIRE(st && done && total, "vqcpc_vocoder_stream_position: null argument");
    *done = st->pos; *total = st->total;
    return VQCPC_OK;
}

extern "C" void vqcpc_vocoder_stream_close(vqcpc_vocoder_stream *st) { delete st; }
