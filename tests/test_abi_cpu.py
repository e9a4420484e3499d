"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/vqcpc.h declares, the ctypes binding (argument types, return types, struct mirrors) agrees
with every declaration, the header is plain C99, the Python mirror keeps the reference's surface,
and the product path fails loudly without a GPU (no fallback)."""
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCC_C99 = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]

SCALARS = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "double": ctypes.c_double, "float": ctypes.c_float}
# every `typedef struct {...} name;` of the header -> its ctypes mirror
MIRRORS = {"vqcpc_encoder_weights": _lib.EncoderWeights, "vqcpc_cpc_weights": _lib.CPCWeights, "vqcpc_vocoder_weights": _lib.VocoderWeights,
           "vqcpc_encoder_front_weights": _lib.EncoderFrontTensors, "vqcpc_encoder_front_grads": _lib.EncoderFrontTensors,
           "vqcpc_vocoder_ar_weights": _lib.VocoderArTensors, "vqcpc_vocoder_ar_grads": _lib.VocoderArTensors,
           "vqcpc_vocoder_cond_weights": _lib.VocoderCondTensors, "vqcpc_vocoder_cond_grads": _lib.VocoderCondTensors,
           "vqcpc_adam_tensor": _lib.AdamTensor, "vqcpc_adam_hyper": _lib.AdamHyper}


@functools.lru_cache(maxsize=None)
def header():
    """include/vqcpc.h without its comments -> (functions, structs).  functions: name -> (return type, [(base type, is pointer)]
    per parameter); structs: name of a ``typedef struct {...} name;`` -> [(base type, is pointer, member, extents)] in order.
    A base type keeps its ``const``: "const float", "int", "vqcpc_encoder"."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vqcpc.h")).read(), flags=re.S)

    def split(decl):                        # "const float *p" / "int64_t *" / "int" -> (base, is pointer, rest)
        m = re.fullmatch(r"\s*((?:const\s+)?\w+)\s*(\**)\s*(.*?)\s*", decl, flags=re.S)
        assert m, decl
        return re.sub(r"\s+", " ", m.group(1)), bool(m.group(2)), m.group(3)

    structs = {}
    for m in re.finditer(r"typedef struct \{([^}]*)\}\s*(\w+);", text):
        members = []
        for decl in filter(str.strip, m.group(1).split(";")):
            first, *more = decl.split(",")
            base, ptr, rest = split(first)
            for p, d in [(ptr, rest)] + [(d.strip().startswith("*"), d.strip().lstrip("* ")) for d in more]:
                name, dims = re.fullmatch(r"(\w+)((?:\[\d+\])*)", d).groups()
                members.append((base, p, name, tuple(int(n) for n in re.findall(r"\d+", dims))))
        structs[m.group(2)] = members
    functions = {}
    for m in re.finditer(r"^((?:const\s+)?\w+\s*\*?)\s*(vqcpc_\w+)\s*\(([^;{}()]*)\)\s*;", text, flags=re.M):
        params = [] if m.group(3).strip() == "void" else [split(p)[:2] for p in m.group(3).split(",")]
        functions[m.group(2)] = (re.sub(r"\s+", " ", m.group(1).replace("*", " *")).strip(), params)
    assert sorted(functions) == sorted(set(re.findall(r"\b(vqcpc_[a-z0-9_]+)\s*\(", text))), "a declaration the parser cannot read"
    return functions, structs


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = sorted(header()[0])
    assert len(names) >= 73
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vqcpc.h but not exported"
    assert sorted(_lib.SYMBOLS) == names and len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    assert _lib.load().vqcpc_abi_version() == 1
    assert "#define VQCPC_ABI_VERSION 1\n" in open(os.path.join(ROOT, "include", "vqcpc.h")).read()
    assert os.listdir(os.path.join(ROOT, "include")) == ["vqcpc.h"]          # one header: a C caller includes it and has everything


def test_argtypes_agree_with_the_header():
    """Every ``argtypes`` list of ``_lib.load()`` against the declaration it binds: a list that is one pointer short, or an ``int``
    bound as 64 bits, shifts every argument behind it -- on the GPU that is a fault, not a failed test."""
    functions, structs = header()
    lib = _lib.load()
    for name, (ret, params) in functions.items():
        f = getattr(lib, name)
        assert len(f.argtypes or ()) == len(params), f"{name}: {len(f.argtypes or ())} argtypes, {len(params)} parameters"
        for k, ((base, ptr), t) in enumerate(zip(params, f.argtypes or ())):
            what = f"{name}, parameter {k} ({base}{' *' if ptr else ''}): {t}"
            if not ptr:
                assert t is SCALARS[base], what
                continue
            assert t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer), what
            if issubclass(t, ctypes._Pointer):
                bare = base.replace("const ", "")
                if bare in structs:
                    assert t._type_ is MIRRORS[bare], what
                elif bare in SCALARS:
                    assert t._type_ is SCALARS[bare], what
        want = {"void": None, "const char *": ctypes.c_char_p, "int": ctypes.c_int}[ret]
        assert f.restype is want, f"{name}: returns {ret}, restype {f.restype}"
    bound = [n for n, f in vars(lib).items() if isinstance(f, lib._FuncPtr) and f.argtypes is not None]
    assert len(bound) >= 70 and not set(bound) - set(_lib.SYMBOLS) - set(_lib.TEST_SYMBOLS)
    assert not set(_lib.TEST_SYMBOLS) & set(_lib.SYMBOLS) and set(_lib.TEST_SYMBOLS) <= set(bound)


def test_structs_mirror_the_header(tmp_path):
    """Every member struct of the header against its ctypes mirror: member names in order, kinds, array extents, and the sizes and
    offsets the C compiler gives."""
    structs = header()[1]
    assert sorted(structs) == sorted(MIRRORS) and len(structs) == 11
    for name, members in structs.items():
        fields = MIRRORS[name]._fields_
        assert [m[2] for m in members] == [n for n, _ in fields], name
        for (base, ptr, member, dims), (_, t) in zip(members, fields):
            got = []
            while hasattr(t, "_length_"):
                got.append(t._length_)
                t = t._type_
            assert tuple(got) == dims and t is (ctypes.c_void_p if ptr else SCALARS[base]), (name, member)
        kinds = {base for base, ptr, _, _ in members if ptr}
        if name.endswith("_weights"):                                # read
            assert kinds == {"const float"}, name
        if name.endswith("_grads"):                                  # written
            assert kinds == {"float"}, name
    assert [(m[0], m[2]) for m in structs["vqcpc_adam_tensor"] if m[1]] == [("float", "param"), ("const float", "grad"), ("float", "exp_avg"),
                                                                         ("float", "exp_avg_sq")]
    vp = ctypes.sizeof(ctypes.c_void_p)
    assert [ctypes.sizeof(c) for c in (_lib.EncoderFrontTensors, _lib.VocoderArTensors, _lib.VocoderCondTensors)] == [17 * vp, 9 * vp, 18 * vp]
    # sizeof and every offsetof, from the C compiler
    src = tmp_path / "layout.c"
    lines = ["    printf(\"%%zu\\n\", sizeof(%s));" % n + "".join("\n    printf(\"%%zu\\n\", offsetof(%s, %s));" % (n, m[2]) for m in ms)
             for n, ms in structs.items()]
    src.write_text('#include "vqcpc.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [v for n, ms in structs.items() for v in [ctypes.sizeof(MIRRORS[n])] + [getattr(MIRRORS[n], m[2]).offset for m in ms]]
    assert got == want


def test_header_is_plain_c(tmp_path):
    """include/vqcpc.h is the drop-in boundary: it must compile as C99 with the calls INTEGRATION.md shows."""
    src = tmp_path / "use.c"
    src.write_text('''#include "vqcpc.h"
#include <stddef.h>
int use(vqcpc_encoder *enc, vqcpc_vocoder *voc, float *p, int64_t *i, void *s) {
    int rc = vqcpc_encoder_encode(enc, p, 1, 32, VQCPC_CONV_AUTO, p, NULL, i, NULL, s);
    rc |= vqcpc_vocoder_generate(voc, i, i, 1, 16, NULL, 13u, 0u, NULL, p, NULL, 0, s);
    return rc;
}
int use_stream(vqcpc_vocoder *voc, float *wav, int64_t *i, void *s) {
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
int use_cpc(const float *w, const float *z, const float *c, const int64_t *u, const int64_t *s, float *out, uint8_t *ok, void *st) {
    vqcpc_cpc_weights cw;
    vqcpc_cpc *cpc = NULL;
    int i, rc;
    for (i = 0; i < 16; ++i) { cw.weight[i] = w; cw.bias[i] = w; }
    cw.n_steps = 6; cw.n_speakers = 8; cw.n_utterances = 8; cw.n_negatives = 17; cw.z_dim = 64; cw.c_dim = 256;
    rc = vqcpc_cpc_create(&cw, &cpc);
    rc |= vqcpc_cpc_score(cpc, z, c, 70, u, s, 13u, 0u, out, out + 1, out + 7, ok, NULL, st);
    rc |= vqcpc_cpc_score(cpc, z, c, 70, NULL, NULL, 13u, 1u, out, out + 1, out + 7, NULL, NULL, st);
    vqcpc_cpc_destroy(cpc);
    return rc;
}
int use_cpc_grad(vqcpc_cpc *cpc, const float *z, const float *c, const float *W, const float *b, const int64_t *u, const int64_t *s,
                 float *out, float *gz, float *gc, float *gW, float *gb, void *st) {
    int rc = vqcpc_cpc_grad(cpc, z, c, 70, W, b, u, s, 13u, 0u, out, out + 1, out + 7, gz, gc, gW, gb, st);
    rc |= vqcpc_cpc_grad(cpc, z, c, 70, NULL, NULL, NULL, NULL, 13u, 1u, out, out + 1, out + 7, NULL, NULL, gW, gb, st);
    return rc;
}
int use_context_grad(vqcpc_encoder *enc, const float *z, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                     float *c, void *saved, const float *gc, float *gz, float *gwi, float *gwh, float *gb, void *st) {
    uint64_t n = 0;
    int rc = vqcpc_encoder_context_saved_bytes(enc, 64, 70, &n);
    rc |= vqcpc_encoder_context_fwd(enc, z, 64, 70, w_ih, w_hh, b_ih, b_hh, c, saved, st);
    rc |= vqcpc_encoder_context_fwd(enc, z, 64, 70, NULL, NULL, NULL, NULL, c, saved, st);
    rc |= vqcpc_encoder_context_bwd(enc, z, 64, 70, w_ih, w_hh, c, saved, gc, gz, gwi, gwh, gb, st);
    rc |= vqcpc_encoder_context_bwd(enc, z, 64, 70, NULL, NULL, c, saved, gc, NULL, gwi, NULL, NULL, st);
    return rc;
}
int use_front_grad(vqcpc_encoder *enc, float *p, void *saved, void *s) {
    vqcpc_encoder_front_weights w;
    vqcpc_encoder_front_grads g;
    uint64_t n = 0;
    int rc = vqcpc_encoder_front_saved_bytes(enc, 1, 32, &n);
    w.conv_weight = p; g.conv_weight = p; w.ln_weight[4] = p; g.ln_bias[0] = NULL;
    rc |= vqcpc_encoder_front_fwd(enc, p, 1, 32, VQCPC_CONV_AUTO, &w, p, saved, s);
    rc |= vqcpc_encoder_front_fwd(enc, p, 1, 32, VQCPC_CONV_AUTO, NULL, p, saved, s);
    rc |= vqcpc_encoder_front_bwd(enc, p, 1, 32, VQCPC_CONV_AUTO, &w, saved, p, &g, s);
    rc |= vqcpc_encoder_vq_bwd(enc, p, p, 16, p, NULL, p, s);
    return rc;
}
int use_vocoder_grad(vqcpc_vocoder *voc, int64_t *i, float *p, double *d, void *saved, void *s) {
    vqcpc_vocoder_ar_weights w;
    vqcpc_vocoder_ar_grads g;
    uint64_t n = 0;
    int rc = vqcpc_vocoder_ar_saved_bytes(voc, 2, 321, &n);
    w.embedding = p; w.w_ih = p; w.w_hh = p; w.b_ih = p; w.b_hh = p; w.fc1_weight = p; w.fc1_bias = p; w.fc2_weight = p; w.fc2_bias = p;
    g = (vqcpc_vocoder_ar_grads){NULL, p, NULL, NULL, NULL, NULL, NULL, NULL, p};
    rc |= vqcpc_vocoder_ar_fwd(voc, i, i, i, 2, 1, 321, NULL, NULL, &w, d, i, i, p, saved, s);
    rc |= vqcpc_vocoder_ar_fwd(voc, i, i, i, 2, 1, 321, NULL, NULL, NULL, d, i, i, NULL, saved, s);
    rc |= vqcpc_vocoder_ar_bwd(voc, i, i, i, 2, 1, 321, NULL, NULL, &w, saved, p, &g, p, s);
    rc |= vqcpc_vocoder_ar_bwd(voc, i, i, i, 2, 1, 321, NULL, NULL, NULL, saved, NULL, NULL, p, s);
    return rc;
}
int use_vocoder_cond_grad(vqcpc_vocoder *voc, int64_t *i, float *p, double *d, void *saved, void *s) {
    vqcpc_vocoder_cond_weights w;
    vqcpc_vocoder_cond_grads g = {0};
    uint64_t n = 0;
    int l, k, rc = vqcpc_vocoder_cond_saved_bytes(voc, 2, 16, &n);
    w.code_embedding = p; w.speaker_embedding = p;
    for (l = 0; l < 2; ++l)
        for (k = 0; k < 2; ++k) { w.prenet_w_ih[l][k] = p; w.prenet_w_hh[l][k] = p; w.prenet_b_ih[l][k] = p; w.prenet_b_hh[l][k] = p; }
    g.code_embedding = p; g.prenet_b_hh[1][1] = p;
    rc |= vqcpc_vocoder_cond_fwd(voc, i, i, 2, 16, NULL, &w, p, saved, s);
    rc |= vqcpc_vocoder_cond_bwd(voc, i, i, 2, 16, NULL, NULL, saved, p, &g, s);
    rc |= vqcpc_vocoder_ar_fwd_cond(voc, i, i, i, 2, 1, 321, NULL, NULL, NULL, p, d, i, i, NULL, saved, s);
    rc |= vqcpc_vocoder_ar_bwd_cond(voc, i, i, i, 2, 1, 321, NULL, NULL, NULL, p, saved, NULL, NULL, p, s);
    return rc;
}
int use_adam(float *p, const float *g, float *m, float *v, void *s) {
    vqcpc_adam_tensor t[2];
    vqcpc_adam_hyper h;
    t[0].param = p; t[0].grad = g; t[0].exp_avg = m; t[0].exp_avg_sq = v; t[0].numel = 64;
    t[1] = t[0]; t[1].numel = 0;
    h.lr = 4e-4; h.beta1 = 0.9; h.beta2 = 0.999; h.eps = 1e-8; h.step = 1;
    return vqcpc_adam_step(t, 2, &h, s) + VQCPC_ADAM_TABLE + VQCPC_ADAM_CHUNK;
}
''')
    r = subprocess.run(GCC_C99 + [str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_state_dict_surface_matches_reference():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    sd = synth.encoder_state_dict()
    assert list(enc.state_dict().keys()) == list(sd.keys())        # SURVEY 8a-1 key set and order
    assert all(enc.state_dict()[k].shape == sd[k].shape for k in sd)
    enc.load_state_dict(sd)
    voc = V.Vocoder(V.ConfVocoder())
    sv = synth.vocoder_state_dict()
    assert set(voc.state_dict().keys()) == set(sv.keys())
    assert all(voc.state_dict()[k].shape == sv[k].shape for k in sv)
    voc.load_state_dict(sv)
    assert isinstance(enc.encoder[-1], torch.nn.Linear)             # encode.py:40 hooks this module


def test_no_cpu_fallback():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256)).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode(torch.zeros(1, 80, 32))
    voc = V.Vocoder(V.ConfVocoder()).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voc.generate(torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    from vectorquantizedcpc_amd import loudness, preprocess         # the front-end drop-ins too
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        preprocess.wave_to_mel(torch.zeros(16000))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loudness.Meter(16000).integrated_loudness(torch.zeros(16000))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loudness.normalize.loudness(torch.zeros(16000), -20.0, -23.0)


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under the product package may import or load it."""
    pkg = os.path.join(ROOT, "vectorquantizedcpc_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", text, flags=re.M), f
                assert "libvqcpc_oracle" not in text, f
            if f.endswith((".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "#include \"../../oracle" not in text and "dlopen" not in text, f


def test_device_memory_has_one_owner():
    """All device and pinned memory of the library is a ``DevBuf`` / ``HostBuf`` (``csrc/common.h``) that frees itself: the
    allocation calls appear in that file only, and no handle struct declares a raw device pointer of its own."""
    csrc = os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc")
    borrowed = set()                  # "struct.member": raw pointers a handle may declare because it does not own them (none today)
    structs = 0
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(csrc, f)).read()
        if f != "common.h":
            found = re.findall(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\b", text)
            assert not found, f"{f}: {sorted(set(found))} outside common.h"
        for m in re.finditer(r"^struct (vqcpc_\w+|LstmPlan) \{\n(.*?)^\};", text, flags=re.M | re.S):
            structs += 1
            for decl in re.finditer(r"\b(?:float|double|unsigned)\s*\*[^;(]*=\s*nullptr[^;]*;", m.group(2)):
                names = re.findall(r"\*\s*(\w+)\s*=\s*nullptr", decl.group(0))
                raw = [n for n in names if f"{m.group(1)}.{n}" not in borrowed]
                assert not raw, f"{f}: struct {m.group(1)} declares raw pointer member(s) {raw}"
    assert structs >= 8               # the seven handle types and LstmPlan were seen


def test_synth_is_deterministic():
    a = synth.encoder_state_dict()["encoder.2.weight"]
    b = synth.encoder_state_dict()["encoder.2.weight"]
    assert torch.equal(a, b)
    assert abs(float(synth.mel("x", 2, 8).mean()) - 0.5) < 0.05


def test_weight_slots_follow_the_module_without_state_dict():
    """The native handles are keyed on (data_ptr, _version) of the weights, read per call through WeightSlots instead of
    state_dict() (71 us vs 5 us): the slots must name exactly the reference's state_dict keys (minus the EMA buffers the
    inference path never reads) and must see load_state_dict, dtype/device moves and buffer replacement."""
    import copy

    import torch

    import vectorquantizedcpc_amd as V
    from vectorquantizedcpc_amd import _lib, synth
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    assert set(enc._WEIGHT_NAMES) == set(enc.state_dict()) - {"codebook.ema_count", "codebook.ema_weight"}
    slots = _lib.WeightSlots(enc, enc._WEIGHT_NAMES)
    k0 = _lib.WeightSlots.key(slots.tensors())
    assert k0 == _lib.WeightSlots.key(slots.tensors())
    enc.load_state_dict(synth.encoder_state_dict())                  # copy_ in place: versions move
    k1 = _lib.WeightSlots.key(slots.tensors())
    assert k1 != k0
    enc.codebook.embedding = torch.zeros(512, 64)                    # a buffer REPLACED by assignment
    k2 = _lib.WeightSlots.key(slots.tensors())
    assert k2 != k1 and slots.tensors()[slots.names.index("codebook.embedding")] is enc.codebook.embedding
    enc.double()                                                     # .to(): parameters keep identity, storage moves
    assert _lib.WeightSlots.key(slots.tensors()) != k2
    voc = V.Vocoder(V.ConfVocoder())
    vs = _lib.WeightSlots(voc, list(voc.state_dict().keys()))
    assert [t.shape for t in vs.tensors()] == [t.shape for t in voc.state_dict().values()]
    assert "_slots" not in copy.deepcopy(enc).__dict__ and copy.deepcopy(enc).codebook._owner() is not enc
    assert voc._WEIGHT_NAMES == list(voc.state_dict().keys())
    # one lifecycle: the three classes take it from _lib.NativeModule and define none of it themselves
    for cls in (V.Encoder, V.CPCLoss, V.Vocoder):
        assert issubclass(cls, _lib.NativeModule) and issubclass(_lib.NativeModule, torch.nn.Module)
        for name in ("_native", "refresh", "__getstate__", "__del__"):
            assert name not in vars(cls) and getattr(cls, name) is getattr(_lib.NativeModule, name), (cls.__name__, name)
