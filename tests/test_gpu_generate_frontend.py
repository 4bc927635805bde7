"""The property the generators' shared prompt stage must keep (music_amd/fast_generate.py: _prime, _first_codes, _note0 in front of
the one launcher): ``generate_codes(net, x[u:u + 1], ...)`` is row u of ``generate_codes_batch(net, x, ...)``, bit for bit, greedy,
for U = 3 different prompts of 16 codes over dilations [1, 2, 4] -

  - on the matrix-core decoder (64 / 64 / 256 channels, Q = 256): as written; corrected recurrence under position windows; with
    classes under windows; with classes under windows and guidance (one pair of rows against three);
  - on the fp32 kernel (filter_width 3, Q = 100, the general plan): the corrected recurrence;

and ``note_num`` 0 and 1 come back as ``(U, note_num)`` / ``(note_num,)`` without a decode launch.  The parameters are scaled as in
tests/class_cond_ref.build: default initialisation gives logits too flat for the two launch forms to agree on every argmax.
Run with -m gpu."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cfg_ref as cr
from tests import class_cond_ref as ref

U, N_CODES, DIL = 3, 16, [1, 2, 4]
MODELS = {
    "mfma": dict(filter_width=2, dilations=DIL, dilation_channels=64, residual_channels=64, skip_channels=256,
                 quantization_channels=256, use_bias=False),
    "mfma_classes": cr.model_case("mfma")["cfg"],
    "fp32": dict(filter_width=3, dilations=DIL, dilation_channels=40, residual_channels=48, skip_channels=96,
                 quantization_channels=100, use_bias=False),
}
assert MODELS["mfma_classes"]["dilations"] == DIL and MODELS["mfma_classes"]["quantization_channels"] == 256


@functools.lru_cache(maxsize=None)
def _net(name):
    """(module on the device, its U prompts)"""
    net = ref.build(MODELS[name], 21).cuda()
    Q = net.quantization_channels
    codes = ref.seed_codes(U, net.receptive_field, Q, 22)
    return net, torch.nn.functional.one_hot(codes, Q).permute(0, 2, 1).float().contiguous().cuda()


def _spy_calls(monkeypatch):
    from music_amd import fast_generate as fg
    seen, real = [], fg.call
    monkeypatch.setattr(fg, "call", lambda fn, *a: seen.append(fn) or real(fn, *a))
    return seen


HALVES = [(0, 128), (128, 256)]
CLASSES = [2, 0, 3]
CASES = {
    "as_written": ("mfma", dict(), "wn_decode_batch_fw"),
    "corrected_windows": ("mfma", dict(correct_queue=True, windows=HALVES, window_pos=3), "wn_win_decode_batch"),
    "classes_windows": ("mfma_classes", dict(correct_queue=True, windows=HALVES, window_pos=3, classes=CLASSES), "wn_win_decode_batch"),
    "classes_windows_guidance": ("mfma_classes", dict(correct_queue=True, windows=HALVES, window_pos=3, classes=CLASSES, guidance=2.0),
                                 "wn_cfg_decode_batch"),
    "fp32_corrected": ("fp32", dict(correct_queue=True), "wn_decode_batch_fw"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_one_utterance_is_its_row_of_the_batch(case, monkeypatch):
    from music_amd import fast_generate as fg
    name, kw, entry = CASES[case]
    net, x = _net(name)
    assert fg._mfma_decode(net._engine_for(x.device)) == (name != "fp32")
    seen = _spy_calls(monkeypatch)
    batch = fg.generate_codes_batch(net, x, N_CODES, **kw)
    assert [s for s in seen if "decode" in s] == [entry]
    assert tuple(batch.shape) == (U, N_CODES) and batch.dtype == torch.int64
    for u in range(U):
        one_kw = dict(kw, classes=[kw["classes"][u]]) if "classes" in kw else kw
        one = fg.generate_codes(net, x[u:u + 1], N_CODES, **one_kw)
        assert tuple(one.shape) == (N_CODES,) and one.dtype == torch.int64
        assert torch.equal(one, batch[u]), (case, u, one.tolist(), batch[u].tolist())
    if "windows" in kw:
        for j in range(N_CODES):
            lo, hi = HALVES[(kw["window_pos"] + j) % 2]
            assert bool(((batch[:, j] >= lo) & (batch[:, j] < hi)).all()), j


@pytest.mark.parametrize("case", ["as_written", "classes_windows_guidance", "fp32_corrected"])
@pytest.mark.parametrize("note_num", [0, 1])
def test_short_requests_launch_no_decode(case, note_num, monkeypatch):
    from music_amd import fast_generate as fg
    name, kw, _ = CASES[case]
    net, x = _net(name)
    full = fg.generate_codes_batch(net, x, 2, **kw)
    seen = _spy_calls(monkeypatch)
    batch = fg.generate_codes_batch(net, x, note_num, **kw)
    one = fg.generate_codes(net, x[:1], note_num, **(dict(kw, classes=kw["classes"][:1]) if "classes" in kw else kw))
    assert not [s for s in seen if "decode" in s]
    assert tuple(batch.shape) == (U, note_num) and tuple(one.shape) == (note_num,) and batch.dtype == one.dtype == torch.int64
    assert torch.equal(batch, full[:, :note_num]) and torch.equal(one, full[0, :note_num])
