"""CPU-side checks of the streaming decode surface (Vocoder.generate_stream): chunk sizes validated before any GPU work.  That
vqcpc_vocoder_stream_* are declared, exported, bound and plain C99: tests/test_abi_cpu.py."""
import pytest

import vectorquantizedcpc_amd as V


@pytest.mark.parametrize("chunk", [0, 100, -160, 160.0, True])
def test_generate_stream_rejects_bad_chunk_sizes_before_gpu_work(chunk):
    import torch
    voc = V.Vocoder(V.ConfVocoder())                     # CPU parameters: any GPU work would raise RuntimeError instead
    z = torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="chunk_samples"):
        voc.generate_stream(z, torch.zeros(1, dtype=torch.int64), chunk_samples=chunk)
    assert voc._handle is None and voc._utterances_done == 0
