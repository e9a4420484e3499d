"""CPU-side checks of the streaming decode surface (vqcpc_vocoder_stream_*, Vocoder.generate_stream): declared, exported, plain
C99, and chunk sizes validated before any GPU work."""
import ctypes
import os
import subprocess

import pytest

import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vqcpc_vocoder_stream_open", "vqcpc_vocoder_stream_next", "vqcpc_vocoder_stream_redo",
         "vqcpc_vocoder_stream_position", "vqcpc_vocoder_stream_close"]


def test_stream_functions_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vqcpc.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert f"{n}(" in header, n
        assert n in _lib.SYMBOLS, n
        assert hasattr(lib, n), n
    assert "typedef struct vqcpc_vocoder_stream vqcpc_vocoder_stream;" in header
    assert _lib.load().vqcpc_vocoder_stream_next.argtypes is not None


def test_stream_header_is_plain_c(tmp_path):
    src = tmp_path / "stream.c"
    src.write_text('''#include "vqcpc.h"
#include <stddef.h>
int use(vqcpc_vocoder *voc, float *wav, int64_t *i, void *s) {
    vqcpc_vocoder_stream *st = NULL;
    int64_t done = 0, total = 0;
    int rc = vqcpc_vocoder_stream_open(voc, i, i, 1, 16, NULL, 13u, 0u, NULL, &st, s);
    if (rc != VQCPC_OK) return rc;
    while (vqcpc_vocoder_stream_position(st, &done, &total) == VQCPC_OK && done < total) {
        rc = vqcpc_vocoder_stream_next(st, 1600, wav, NULL, s);
        if (rc == VQCPC_OK && vqcpc_vocoder_check(voc) != VQCPC_OK) rc = vqcpc_vocoder_stream_redo(st, wav, NULL, s);
        if (rc != VQCPC_OK) break;
    }
    vqcpc_vocoder_stream_close(st);
    return rc;
}
''')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("chunk", [0, 100, -160, 160.0, True])
def test_generate_stream_rejects_bad_chunk_sizes_before_gpu_work(chunk):
    import torch
    voc = V.Vocoder(V.ConfVocoder())                     # CPU parameters: any GPU work would raise RuntimeError instead
    z = torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="chunk_samples"):
        voc.generate_stream(z, torch.zeros(1, dtype=torch.int64), chunk_samples=chunk)
    assert voc._handle is None and voc._utterances_done == 0
