"""-m gpu: the HIP resampler (vqcpc_resampler_*, preprocess.resample) against the float64 oracle.
PARITY UNPINNED (resampy / librosa absent): oracle/resample_ref.py restates the published kaiser_best algorithm.
Tolerance: the kernel replays the reference's accumulated output clock (time_register += time_increment, summed once on the
host) and sums both wings in float64 in the reference's order, then rounds once to float32.  So every output is within one
float32 ulp of float32(want) (1e-12 absolute where the sum cancels) and at least 99.9 % are bit-equal
(resample_ref.compare_rounded; tests/test_gpu_resample_f64.py holds the wider cases and what the MI355X showed).  Until the
kernel had that clock these tests allowed 2e-6 absolute."""
import numpy as np
import pytest
import torch

from oracle import resample_ref as R
from vectorquantizedcpc_amd import io, preprocess, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 16000), (48000, 16000), (22050, 16000), (8000, 16000), (16000, 22050)])
def test_resample_matches_oracle(sr_in, sr_out):
    n = 3000
    x = (synth.uniform01(f"rs/{sr_in}", n) * 2 - 1).astype(np.float32)
    x = np.convolve(x, np.ones(5) / 5, mode="same").astype(np.float32)
    got = preprocess.resample(torch.from_numpy(x).cuda(), sr_in, sr_out).cpu().numpy()
    want = R.resample(x, sr_in, sr_out)
    assert got.shape == want.shape and got.dtype == np.float32
    ok, share, ulp, _ = R.compare_rounded(got, want)
    print("\nresample %d->%d: max ulp %d, bit-equal %.5f, max |diff| %.2e" % (sr_in, sr_out, ulp, share, np.abs(got - want).max()))
    assert ok and share >= 0.999, (ulp, share)


def test_ragged_batch_and_load_wav(tmp_path):
    lens = [2000, 777, 1]
    x = np.zeros((3, 2000), np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = (synth.uniform01(f"rsb/{b}", n) - 0.5).astype(np.float32)
    got = preprocess.resample(torch.from_numpy(x).cuda(), 44100, 16000, lengths=lens).cpu().numpy()
    assert got.shape == (3, int(np.ceil(2000 * 16000 / 44100)))
    for b, n in enumerate(lens):
        want = R.resample(x[b, :n], 44100, 16000)
        ok, share, _, _ = R.compare_rounded(got[b, : len(want)], want)
        assert ok and share >= 0.999 and not got[b, len(want):].any()
    from scipy.io import wavfile
    wavfile.write(tmp_path / "a.wav", 22050, x[0])
    w = io.load_wav(tmp_path / "a", 16000)
    assert w.shape == (int(np.ceil(2000 * 16000 / 22050)),) and not w.is_cuda
    ok, share, _, _ = R.compare_rounded(w.numpy(), R.resample(x[0], 22050, 16000))
    assert ok and share >= 0.999
    wavfile.write(tmp_path / "b.wav", 16000, x[0])
    assert torch.equal(io.load_wav(tmp_path / "b", 16000), torch.from_numpy(x[0]))
