"""CPU checks of the one decode call path: fast_generate._decode_call writes the argument list and chooses the entry point, and
_lib composes the decode signatures from shared pieces.  Nothing is launched."""
import ctypes

import pytest

P = 1 << 20            # "some non-NULL address"
NO_TABLES = (None, 0, None, 0, None, None, 1, 0)
TABLES = (P, 2 * 3 * 128, P, 3 * 256, P, P, 3, -3)


def _call(fg, smp, cond):
    return fg._decode_call((2, 4, 64, 64, 256, 256), P, P, P, (P, None, P, 4096, None, P, None, P, None),
                           (P, P, P, P, None, P, None), 0, 12, 1, P, 3, 960, smp, (P, 0, 8, 16, 24, 32, 40), cond)


@pytest.mark.parametrize("sampling", ["plain", "filtered", "table"])
@pytest.mark.parametrize("cond", [None, NO_TABLES, TABLES], ids=["unconditioned", "cond-origin-no-tables", "cond-origin-tables"])
def test_decode_call_chooses_the_entry_and_nests_the_argument_lists(sampling, cond):
    import torch
    from music_amd import _lib
    from music_amd import fast_generate as fg
    kw = {"plain": dict(temperature=0.8, top_k=None), "filtered": dict(temperature=0.8, top_k=40),
          "table": dict(temperature=[0.5, 0.8, 1.0], top_k=[0, 40, 5])}[sampling]
    smp = fg._Sampling(3, kw["temperature"], kw["top_k"], None, 7, None, torch.device("cpu"))
    assert smp.plain == (sampling == "plain") and (smp.table is not None) == (sampling == "table")
    name, args = _call(fg, smp, cond)
    want = "wn_decode_batch_samp" if sampling != "plain" else "wn_decode_batch_fw" if cond is None else "wn_decode_batch_cond"
    assert name == want
    assert len(args) + 1 == len(_lib.SIGNATURES[name])
    # the samp tuple begins with the cond tuple, which begins with the fw tuple (the launch's own settings aside)
    plain = fg._Sampling(3, kw["temperature"] if sampling != "table" else 0.0, None, None, 7 if sampling != "table" else 0, None,
                         torch.device("cpu"))
    fw = _call(fg, plain, None)
    co = _call(fg, plain, cond if cond is not None else NO_TABLES)
    assert fw[0] == "wn_decode_batch_fw" and co[0] == "wn_decode_batch_cond"
    assert co[1][:len(fw[1])] == fw[1] and args[:len(fw[1])] == fw[1]
    if name != "wn_decode_batch_fw":
        assert args[:len(co[1])] == co[1]
        assert co[1][len(fw[1]):] == (cond if cond is not None else NO_TABLES)
    if name == "wn_decode_batch_samp":
        assert args[len(co[1]):] == (smp.table.data_ptr() if sampling == "table" else None, 40 if sampling == "filtered" else 0, 1.0)
    # every argument converts under the bound signature
    for v, t in zip(args, _lib.SIGNATURES[name]):
        t(v)


def test_decode_signatures_equal_the_written_out_lists():
    """The composition in _lib (head + batch + pk + conditioning + sampling tails, stream last) against the lists as they were
    written out one by one."""
    from music_amd import _lib
    _p, _i, _l, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    literal = {
        "wn_decode": [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l,
                      _i, _i, _p, _p],
        "wn_decode_batch": [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l,
                            _i, _i, _p, _i, _l, _f, _l, _p],
        "wn_decode_sync_granules": [_i, _i, _i],
        "wn_decode_batch_pk": [_i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _l,
                               _i, _i, _p, _i, _l, _f, _l, _p, _l, _l, _l, _l, _l, _l, _p],
        "wn_decode_batch_fw": [_i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                               _l, _i, _i, _p, _i, _l, _f, _l, _p, _l, _l, _l, _l, _l, _l, _p],
        "wn_decode_batch_cond": [_i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                 _l, _i, _i, _p, _i, _l, _f, _l, _p, _l, _l, _l, _l, _l, _l, _p, _l, _p, _l, _p, _p, _i, _l, _p],
        "wn_decode_batch_samp": [_i, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                 _l, _i, _i, _p, _i, _l, _f, _l, _p, _l, _l, _l, _l, _l, _l, _p, _l, _p, _l, _p, _p, _i, _l,
                                 _p, _i, _f, _p],
    }
    assert sorted(k for k in _lib.SIGNATURES if k.startswith("wn_decode")) == sorted(literal)
    for name, sig in literal.items():
        assert _lib.SIGNATURES[name] == sig, name
