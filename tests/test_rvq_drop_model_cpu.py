"""CPU checks of quantiser dropout (`vq_stage_dropout`, music_amd/vq_dropout.py) on the module surface and the host-side rules, in the
pattern of tests/test_rvq_model_cpu.py: the constructor's refusals, the draw (a pure function of seed, step and GLOBAL clip index, so
every data-parallel layout draws the same counts), what `stages=` may be, which -1 patterns decode_codes accepts - all decided on the
host, before the library is needed -, and that the key adds nothing to state_dict.  No device is touched."""
import json
import math

import numpy as np
import pytest
import torch

from tests.test_vq_model_cpu import CFG, VQ, _equal, _net

S = 4
RVQ = dict(VQ, vq_stages=S)


def test_constructor_refusals_and_defaults():
    for p in (-0.1, 1.5, True, False, "0.5", None, float("nan")):
        with pytest.raises(ValueError, match="vq_stage_dropout"):
            _net(**dict(RVQ, vq_stage_dropout=p))
    for kw in (VQ, dict(VQ, vq_stages=1), {}):
        with pytest.raises(ValueError, match="vq_stage_dropout > 0 requires vq_stages > 1"):
            _net(**dict(kw, vq_stage_dropout=0.5))
    assert _net(**RVQ).vq_stage_dropout == 0.0 and _net(vq_stage_dropout=0.0).vq_stage_dropout == 0.0      # off needs no quantiser
    for p in (0, 0.5, 1, 1.0):
        assert _net(**dict(RVQ, vq_stage_dropout=p)).vq_stage_dropout == float(p)
    from music_amd.model1 import wavenet_autoencoder
    params = json.loads(json.dumps(dict(CFG, **dict(RVQ, vq_stage_dropout=0.5))))                           # as model_params.json gives it
    assert wavenet_autoencoder(**params).vq_stage_dropout == 0.5


@pytest.mark.parametrize("update", ["gradient", "ema"])
def test_the_key_adds_no_parameter_no_buffer_and_no_rng_draw(update):
    kw = dict(RVQ, vq_update=update)
    torch.manual_seed(5)
    a = _net(**kw)
    rng_a = torch.get_rng_state()
    b = _net(vq_stage_dropout=0.5, **kw)
    rng_b = torch.get_rng_state()
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(_equal(sa[k], sb[k]) for k in sa) and torch.equal(rng_a, rng_b)
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    b.load_state_dict(sa), a.load_state_dict(sb)                                   # checkpoints load both ways
    b.draw_stages(8)
    assert list(b.state_dict()) == list(sa) and b.vq_dropout_calls == 1           # the counter is a plain attribute
    assert a.draw_stages(8) is None and a.vq_dropout_calls == 0                    # off: nothing is drawn


def test_the_draw_is_a_pure_function_of_seed_step_and_global_clip():
    from music_amd.vq_dropout import draw_stages
    whole = draw_stages(3, 17, 0, 16, 8, 0.5)
    assert whole.dtype == np.int32 and whole.shape == (16,) and np.array_equal(whole, draw_stages(3, 17, 0, 16, 8, 0.5))
    for world in (2, 8):                                                            # one rank, or split over 2 or 8: the same counts
        per = 16 // world
        assert np.array_equal(np.concatenate([draw_stages(3, 17, r * per, per, 8, 0.5) for r in range(world)]), whole)
    ragged = [draw_stages(3, 17, lo, hi - lo, 8, 0.5) for lo, hi in ((0, 6), (6, 12), (12, 16), (16, 16))]
    assert np.array_equal(np.concatenate(ragged), whole) and ragged[-1].shape == (0,)
    big = draw_stages(3, 17, 0, 4096, 8, 0.5)
    assert not np.array_equal(big, draw_stages(4, 17, 0, 4096, 8, 0.5))            # the seed, the step and the clip all matter
    assert not np.array_equal(big, draw_stages(3, 18, 0, 4096, 8, 0.5))
    assert not np.array_equal(big[:-1], big[1:])
    assert np.array_equal(draw_stages(1 << 70, 1 << 40, 1 << 33, 5, 8, 1.0), draw_stages(1 << 70, 1 << 40, 1 << 33, 5, 8, 1.0))
    for bad in (dict(S=0), dict(p=1.5), dict(p=-0.1), dict(p=True), dict(B=-1), dict(step=-1)):
        with pytest.raises(ValueError):
            draw_stages(**dict(dict(seed=0, step=0, first_clip=0, B=4, S=4, p=0.5), **bad))


def test_the_draw_has_the_distribution_the_key_describes():
    from music_amd.vq_dropout import draw_stages
    N = 4096
    for s in (2, 4, 8):
        assert (draw_stages(0, 0, 0, N, s, 0.0) == s).all()                         # p = 0: all S
        n = draw_stages(0, 1, 0, N, s, 1.0)                                          # p = 1: uniform over 1 .. S
        assert sorted(set(n.tolist())) == list(range(1, s + 1))
        # p = 0.5: a clip keeps all S with probability q = 1/2 + 1/(2 S), inside [0.5, 0.5 + 0.5 / S].  The count over N draws is
        # binomial with sigma = sqrt(q (1 - q) / N) <= 1 / (2 sqrt(N)) = 1/128; 5 sigma (two-sided 6e-7) is the margin
        share = float((draw_stages(0, 2, 0, N, s, 0.5) == s).mean())
        margin = 5.0 * 0.5 / math.sqrt(N)
        assert 0.5 - margin <= share <= 0.5 + 0.5 / s + margin, (s, share)
        assert abs(share - (0.5 + 0.5 / s)) <= margin, (s, share)
        # and among p = 1 draws every value has about N / S: sigma <= sqrt(N / S), 5 sigma again
        counts = np.bincount(n, minlength=s + 1)[1:]
        assert (np.abs(counts - N / s) <= 5.0 * math.sqrt(N / s)).all(), counts
    net = _net(**dict(RVQ, vq_stage_dropout=1.0))
    net.vq_dropout_seed = 9
    a, b = net.draw_stages(64), net.draw_stages(64)                                 # the module's counter: steps 0 and 1
    assert np.array_equal(a, draw_stages(9, 0, 0, 64, S, 1.0)) and np.array_equal(b, draw_stages(9, 1, 0, 64, S, 1.0))
    assert np.array_equal(net.draw_stages(8, step=5, first_clip=24), draw_stages(9, 5, 0, 64, S, 1.0)[24:32]) and net.vq_dropout_calls == 2


def test_what_stages_may_be():
    from music_amd.vq_dropout import stage_counts
    assert stage_counts(None, 3, S) is None
    for given in (2, np.int64(2), [2, 2, 2], (2, 2, 2), np.array([2, 2, 2]), torch.tensor([2, 2, 2]), torch.tensor(2)):
        n = stage_counts(given, 3, S)
        assert n.dtype == np.int32 and n.tolist() == [2, 2, 2], given
    assert stage_counts([1, S, 2], 3, S).tolist() == [1, S, 2] and stage_counts(S, 2, S).tolist() == [S, S]
    for bad in (0, S + 1, -1, True, 2.0, "2", [1, 2], [1, 2, 3, 4], [1, 0, 2], [1, S + 1, 2], [1.0, 2.0, 3.0], [True, True, True],
                torch.tensor([1.0, 2.0, 3.0]), np.array([[1, 2, 3]]), {1, 2, 3}):
        with pytest.raises(ValueError, match="stages"):
            stage_counts(bad, 3, S)
    # a model of ONE stage (or without a quantiser): only what means "all stages" passes, and means the launches without dropout
    assert stage_counts(1, 3, 1) is None and stage_counts([1, 1, 1], 3, 1) is None
    for bad in (2, [1, 2, 1], 0):
        with pytest.raises(ValueError, match="stages"):
            stage_counts(bad, 3, 1)


def test_the_module_refuses_bad_stages_before_an_engine_is_built():
    x = torch.zeros(2, 256, 64)
    for net, bad in ((_net(**RVQ), S + 1), (_net(**RVQ), [1, 2, 3]), (_net(**RVQ), 1.5), (_net(**VQ), 2), (_net(), [2, 2])):
        with pytest.raises(ValueError, match="stages"):
            net(x, stages=bad)
        assert net._engine is None
    with pytest.raises(RuntimeError, match="no CPU path"):                          # a good value gets as far as the device check
        _net(**RVQ)(x, stages=[1, S])


def test_which_absent_stage_patterns_decode_codes_accepts():
    from music_amd.vq_dropout import counts_of_codes
    B, Le = 3, 5
    codes = torch.arange(B * S * Le).reshape(B, S, Le) % 7
    assert counts_of_codes(codes, S) is None and counts_of_codes(codes[:, :2], S) is None       # no -1: a plain prefix, the old path
    c = codes.clone()
    c[0, 1:], c[2, 3:] = -1, -1
    assert counts_of_codes(c, S).tolist() == [1, S, 3] and counts_of_codes(c, S).dtype == np.int32
    assert counts_of_codes(c[:, :3], S).tolist() == [1, 3, 3]                        # (B, n, Le) with n < S
    assert counts_of_codes(c.numpy(), S).tolist() == [1, S, 3]

    def refused(change, match):
        w = codes.clone()
        change(w)
        with pytest.raises(ValueError, match=match):
            counts_of_codes(w, S)

    refused(lambda w: w[1, 2, 3].fill_(-1), "same in all of its frames")             # one frame alone
    refused(lambda w: w[1, 0].fill_(-1), "stage 0")                                  # stage 0 absent
    refused(lambda w: w[1].fill_(-1), "stage 0")
    refused(lambda w: w[1, 1].fill_(-1), "suffix")                                   # a hole: stage 1 absent, 2 and 3 present
    refused(lambda w: w[1, 2].fill_(-2), "below -1")
    for bad in (codes[:, 0], codes[:, :0], torch.cat([codes, codes[:, :1]], 1), codes.float()):
        with pytest.raises(ValueError):
            counts_of_codes(bad, S)
