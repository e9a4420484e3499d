"""-m gpu: the gradients of the vocoder's conditioning path (``csrc/prenet_grad.hip``, ``vqcpc_vocoder_cond_fwd`` / ``_bwd``) -- the
eighteen gradients of ``code_embedding``, ``speaker_embedding`` and ``rnnms.prenet`` against float64 on the eleven cases of
tests/cond_grad_ref.py, the forward's bits against ``Vocoder.condition`` and ``vqcpc_vocoder_ar_fwd``, the ``*_cond`` forms of the
scoring entries against the plain ones, partial requests, repeatability on a dirty work space, a bad index -- and the chain: all 27
gradients of the vocoder objective (``Vocoder.vocoder_gradients``, ``Vocoder.nll(..., differentiable=True, train=...)``) against the
float64 end-to-end loss.

Cases, reference and judge: tests/cond_grad_ref.py and tests/grad_judge.py (``judge`` prints every figure, then asserts): per tensor
``max |G - G64| <= 4 max(e_ref, 2^-24 max |G64|)``.  The reference runs every utterance alone on its own frames, so a ragged batch
that passes equals its utterances one at a time, in value.  Nothing here is measured on the code under test.

Observed on an MI355X, largest err / bound over the eleven cases: the tables 0.346 (speaker_embedding, ``long``), w_ih 0.332, w_hh
0.567 (layer 1 reverse, ``sparse_upstream``), b_ih 0.371, b_hh 0.393; over the three chain cases 0.226 among the eighteen conditioning
tensors and 0.289 among the nine of rnnms.ar.
"""
import numpy as np
import pytest
import torch

import cond_grad_ref as R
import voc_grad_ref as VR
import vectorquantizedcpc_amd as V

pytestmark = pytest.mark.gpu

_voc = {}


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def vocoder(c, fresh=False):
    """The Vocoder of a case's sizes and weight set on the GPU; shared per size and weight set unless ``fresh``."""
    key = (c["dz"], c["ds"], c["C"], c["weights"])
    if fresh or key not in _voc:
        v = V.Vocoder(V.ConfVocoder(dim_i_embedding=c["dz"], dim_speaker_embedding=c["ds"], rnnms=V.ConfRNNMSVocoder(
            dim_i_feature=c["dz"] + c["ds"], dim_voc_latent=c["C"], wave_ar=V.ConfWaveAR(size_h_rnn=512))))
        v.load_state_dict(c["sd"])
        v = v.to("cuda").eval()
        if fresh:
            return v
        _voc[key] = v
    return _voc[key]


def run(voc, c, **kw):
    return voc.cond_gradients(c["z"].cuda(), c["spk"].cuda(), c["G"].cuda(), n_codes=c["n_codes"], **kw)


def chain_vocoder(c):
    v = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(dim_voc_latent=c["C"], upsampling_t=c["up"],
                                                         wave_ar=V.ConfWaveAR(size_i_embed_ar=c["de"], size_h_rnn=c["Hr"]))))
    v.load_state_dict(c["sd"])
    v = v.to("cuda").eval()
    for k, o in c["options"].items():
        v.set_option(k, o)
    return v


def chain_inputs(c):
    return (c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda()), dict(lengths=c["lengths"], n_codes=c["n_codes"])


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_gradients_against_float64(name):
    c = R.load(name)
    got = run(vocoder(c), c)
    host = {k: got[k].cpu().numpy() for k in R.KEYS + ("cond",)}
    code, spk = host["code_embedding.weight"], host["speaker_embedding.weight"]
    named = sorted({int(k) for b, n in enumerate(c["n_codes"]) for k in c["z"][b, :n]})
    speakers = sorted({int(s) for s, n in zip(c["spk"], c["n_codes"]) if n})
    if c["upstream"] != "dense":                                     # only that utterance contributes: every other sum is exact
        b = c["upstream"][0]
        named, speakers = sorted({int(k) for k in c["z"][b, :c["n_codes"][b]]}), [int(c["spk"][b])]
    # rows of codes and speakers that the batch never names: +0, bit for bit
    assert not code[[k for k in range(R.N_CODES) if k not in named]].view(np.uint32).any()
    assert not spk[[s for s in range(R.N_SPK) if s not in speakers]].view(np.uint32).any()
    assert all(code[k].any() for k in named) and all(spk[s].any() for s in speakers)
    for b, n in enumerate(c["n_codes"]):                             # +0 past an utterance's frames
        assert not host["cond"][b, 2 * n:].view(np.uint32).any(), b
    R.judge(name, host, "GPU")


# ------------------------------------------------------------------ 2. the forward is the conditioning of every other entry
@pytest.mark.parametrize("name", ["ref_sizes", "ragged", "hp64", "b17"])
def test_forward_bits(name):
    c = R.load(name)
    voc = vocoder(c)
    z, spk = c["z"].cuda(), c["spk"].cuda()
    nc = V._lib.int_array(c["n_codes"], c["B"], "n_codes")
    own = voc._cond_fwd(z, spk, nc, None)[0]                                                # NULL: the handle's copies
    mine = voc._cond_fwd(z, spk, nc, voc._cond_weights(voc._cond_params(), z.device))[0]    # the caller's pointers
    assert torch.equal(bits(own), bits(mine))
    if c["n_codes"] == [c["Tc"]] * c["B"]:
        assert torch.equal(bits(own), bits(voc.condition(z, spk)))
    # the cond output of vqcpc_vocoder_ar_fwd (ragged rows): every utterance scores one step, so that the scan's conditioning runs
    live = [b for b, n in enumerate(c["n_codes"]) if n]
    audio = torch.zeros(c["B"], 2, dtype=torch.int64, device="cuda")
    call = voc._nll_call(audio, z, spk, [2 if n else 0 for n in c["n_codes"]], c["n_codes"])
    cond = voc._ar_fwd(call, None, want_cond=True)[3]
    assert live and torch.equal(bits(own), bits(cond))
    voc.check()


def test_forward_with_moved_weights_has_the_bits_of_a_handle_made_from_them():
    c = R.load("ragged")
    voc = vocoder(c, fresh=True)
    z, spk, G = c["z"].cuda(), c["spk"].cuda(), c["G"].cuda()
    voc.condition(z, spk)                                            # a live handle with the old weights
    handle = voc._handle.value
    moved = [p.detach() * 1.25 for p in voc._cond_params()]
    got = voc.cond_gradients(z, spk, G, n_codes=c["n_codes"], weights=moved)
    assert voc._handle.value == handle
    other = vocoder(c, fresh=True)
    with torch.no_grad():
        for p, w in zip(other._cond_params(), moved):
            p.copy_(w)
    nc = V._lib.int_array(c["n_codes"], c["B"], "n_codes")
    cond, saved = other._cond_fwd(z, spk, nc, None)                  # NULL: the copies of a handle created from the moved tensors
    grads = other._cond_bwd(z, spk, nc, saved, G, None)
    assert torch.equal(bits(got["cond"]), bits(cond))
    for k, g in zip(R.KEYS, grads):
        assert torch.equal(bits(got[k]), bits(g)), k
    other.check()


@pytest.mark.parametrize("name", ["ragged", "h512"])
def test_scoring_entries_with_the_series_given_have_the_bits_of_the_plain_ones(name):
    c = VR.load(name)
    voc = chain_vocoder(c)
    args, lens = chain_inputs(c)
    call = voc._nll_call(*args, lens["lengths"], lens["n_codes"])
    cond_in = voc._cond_fwd(call[1], call[2], call[7], None)[0]
    for ws in (None, voc._ar_weights(voc._ar_params(), args[0].device)):
        plain = voc._ar_fwd(call, ws, want_cond=True)
        given = voc._ar_fwd(call, ws, want_cond=True, cond_in=cond_in)
        for a, b in zip(plain[:4], given[:4]):
            assert torch.equal(bits(a), bits(b))
        g0, gc0 = voc._ar_bwd(call, plain[4], ws, cond_grad=True)
        g1, gc1 = voc._ar_bwd(call, given[4], ws, cond_grad=True, cond_in=cond_in)
        assert torch.equal(bits(gc0), bits(gc1)) and gc0.any()
        for k, a, b in zip(VR.KEYS, g0, g1):
            assert torch.equal(bits(a), bits(b)), k
    voc.check()


# ------------------------------------------------------------------ 3. partial requests
@pytest.mark.parametrize("name", ["ragged", "dz_ne_ds"])
def test_partial_requests_give_the_bits_of_the_full_call(name):
    c = R.load(name)
    voc = vocoder(c)
    full = run(voc, c)
    layer1 = tuple(k for k in R.KEYS if "_l1" in k)
    biases = tuple(k for k in R.KEYS if "bias" in k)
    for want in (layer1, ("code_embedding.weight",), biases, ("speaker_embedding.weight", "rnnms.prenet.weight_hh_l0_reverse")):
        part = run(voc, c, want=want)
        assert {k for k in R.KEYS if k in part} == set(want)
        for k in want:
            assert torch.equal(bits(part[k]), bits(full[k])), (want, k)
    with pytest.raises(RuntimeError, match="no wanted output"):
        run(voc, c, want=())


# ------------------------------------------------------------------ 4. equal inputs, equal bits, on a work space that is dirty
def test_repeatable_on_a_dirty_work_space():
    small, large = R.load("ragged"), R.load("b17")
    voc = vocoder(small, fresh=True)
    first = run(voc, small)
    before = voc.workspace_bytes()
    run(voc, large)                                                  # another shape: the work space is left full of it
    second = run(voc, small)
    voc.cond_gradients(large["z"].cuda(), large["spk"].cuda(), torch.full_like(large["G"], float("nan")).cuda())      # NaN through dOut, dgi, dgh, the carry, dseries
    third = run(voc, small)
    for k in R.KEYS + ("cond",):
        assert torch.equal(bits(first[k]), bits(second[k])) and torch.equal(bits(first[k]), bits(third[k])), k
        assert torch.isfinite(third[k]).all(), k
    assert voc.workspace_bytes() >= before


def test_a_bad_index_raises_and_is_not_left_latched():
    c = R.load("b1")
    voc = vocoder(c, fresh=True)
    z, spk, G = c["z"].cuda(), c["spk"].cuda(), c["G"].cuda()
    bad = z.clone()
    bad[0, 1] = R.N_CODES
    with pytest.raises(IndexError):
        voc.cond_gradients(bad, spk, G)
    with pytest.raises(IndexError):
        voc.cond_gradients(z, torch.tensor([-1], device="cuda"), G)
    good = voc.cond_gradients(z, spk, G)                             # nothing latched: the next call is clean
    want = run(vocoder(c), c)
    for k in R.KEYS:
        assert torch.equal(bits(good[k]), bits(want[k])), k


# ------------------------------------------------------------------ 5. the chain: all 27 tensors of the vocoder objective
@pytest.mark.parametrize("name", R.CHAIN_CASES)
def test_chain_against_float64_and_the_autograd_surface(name):
    c = VR.load(name)
    voc = chain_vocoder(c)
    args, lens = chain_inputs(c)
    got = voc.vocoder_gradients(*args, **lens, grad_loss=c["grad_loss"])
    ref = R.chain64(name)
    print(f"GPU chain {name}: loss {float(got['loss']):.9f}, float64 {float(ref['loss']):.9f}")
    assert set(R.ALL27) <= set(got) and len(R.ALL27) == 27
    host = {k: got[k].cpu().numpy() for k in R.ALL27}
    R.judge_chain(name, host, "GPU")
    # the scoring half is vqcpc_vocoder_ar_fwd / _bwd's: the bits of ar_gradients
    ar = voc.ar_gradients(*args, **lens, grad_loss=c["grad_loss"])
    assert torch.equal(bits(got["nll_sum"]), bits(ar["nll_sum"]))
    for k, n in zip(VR.KEYS, R.AR_NAMES):
        assert torch.equal(bits(got[n]), bits(ar[k])), k
    # an utterance that scores nothing reads no frame: its rows of grad_cond are +0 and its codes receive exact zero
    code = host["code_embedding.weight"]
    read = set()
    for b, (n, nc) in enumerate(zip(c["slen"], c["n_codes"])):
        frames = min((n + c["up"] - 1) // c["up"], 2 * nc)
        read |= {int(k) for k in c["z"][b, :nc]} if frames else set()
    assert not code[[k for k in range(R.N_CODES) if k not in read]].view(np.uint32).any()

    # nll(differentiable=True, train=all three).loss.backward(): the bits of vocoder_gradients
    voc.zero_grad(set_to_none=True)
    res = voc.nll(*args, **lens, differentiable=True, train=("ar", "prenet", "embeddings"))
    assert res.loss.requires_grad and torch.equal(bits(res.nll_sum), bits(got["nll_sum"]))
    (res.loss * (1.0 if c["grad_loss"] is None else c["grad_loss"])).backward()
    params = dict(voc.named_parameters())
    for k in R.ALL27:
        assert torch.equal(bits(params[k].grad), bits(got[k])), k
    # train=("prenet",): only the sixteen prenet tensors receive a gradient
    voc.zero_grad(set_to_none=True)
    voc.nll(*args, **lens, differentiable=True, train=("prenet",)).loss.backward()
    for k in R.ALL27:
        if k.startswith("rnnms.prenet."):
            assert torch.equal(bits(params[k].grad), bits(got[k])), k
        else:
            assert params[k].grad is None, k
    # the default leaves the conditioning path without a gradient
    voc.zero_grad(set_to_none=True)
    voc.nll(*args, **lens, differentiable=True).loss.backward()
    assert all((params[k].grad is None) == (not k.startswith("rnnms.ar.")) for k in R.ALL27)


def test_five_adam_steps_over_all_27_tensors_on_one_handle():
    c = VR.load("ragged")
    voc = chain_vocoder(c)
    args, lens = chain_inputs(c)
    voc.nll(*args, **lens)
    opt = torch.optim.Adam(voc.parameters(), lr=1e-3)
    handles, values = set(), []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = voc.nll(*args, **lens, differentiable=True, train=V.Vocoder.TRAIN_PARTS).loss
        loss.backward()
        opt.step()
        handles.add(voc._handle.value)
        values.append(float(loss.detach()))
    print("five Adam steps over all 27 tensors:", values)
    assert len(handles) == 1 and all(a > b for a, b in zip(values, values[1:])), values
    assert len(list(voc.parameters())) == 27 and all(p.grad is not None for p in voc.parameters())
    fresh = voc.nll(*args, **lens)                                   # through _native(): rebuilt once, reads the stepped weights
    assert float(fresh.loss) < values[-1]
