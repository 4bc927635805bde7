"""CPU checks of the EMA shadow weights: the entry point wn_ema_flat (include/wavenet_hip.h) - declared, exported, bound, every
refusal reported by name before anything is launched - and its host surface (music_amd/ema.py, the optimizers of music_amd/train.py
and music_amd/ae_train.py on torch's own path, the engines' step with the launches patched out, swapped(), checkpoint rotation).
No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.ema_ref import Ref64, kernel_w
from tests.helpers import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


def test_entry_is_declared_exported_and_bound_and_the_version_stays_9():
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint wn_ema_flat\s*\((.*?)\);", src, flags=re.S)
    assert decl, "wn_ema_flat is not declared"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wn_ema_flat")
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["wn_ema_flat"]) == 8
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().wn_version()


def test_load_names_a_symbol_an_older_library_lacks(monkeypatch):
    from music_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "wn_not_in_this_library", [])
    with pytest.raises(_lib.WavenetHipError, match="wn_not_in_this_library"):
        _lib.load()


def test_refusals_are_reported_by_name_and_empty_calls_pass():
    from music_amd import _lib
    lib = _lib.load()
    P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch
    nan = float("nan")

    def bad(arg, *args):
        rc = lib.wn_ema_flat(*args)
        msg = lib.wn_last_error().decode()
        assert rc == -4 and "wn_ema_flat" in msg and ("'%s'" % arg in msg or " %s " % arg in msg), (arg, rc, msg)

    #     ema p  n  decay warmup t state stream
    ok = [P, P, 8, 0.999, 1, 1, None, None]

    def case(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[("ema", "p", "n", "decay", "warmup", "t", "state").index(k)] = v
        return a
    bad("n", *case(n=-1))
    bad("ema", *case(ema=None))
    bad("p", *case(p=None))
    bad("ema", *case(ema=P + 2))
    bad("p", *case(p=P + 1))
    bad("state", *case(state=P + 4))
    for d in (1.0, -0.25, 1.5, nan):
        bad("decay", *case(decay=d))
    bad("t", *case(t=0))
    bad("t", *case(t=-3))
    # n == 0: nothing to do, NULLs allowed, whatever the other arguments are
    assert lib.wn_ema_flat(None, None, 0, 0.999, 0, 1, None, None) == 0
    assert lib.wn_ema_flat(None, None, 0, nan, 1, 0, None, None) == 0


def test_json_keys_and_unset_means_none():
    from music_amd import ae_train, ema
    from music_amd import train as T
    assert ema.ema_options({}) == (None, False)
    assert ema.ema_options({"ema_decay": 0.999, "ema_warmup": 1}) == (0.999, True)
    assert ema.make(None) is None
    lin = torch.nn.Linear(3, 2)
    for kind in ("adam", "sgd", "rmsprop"):
        assert T.get_optimizer(lin, kind, 1e-3, 0.9).ema is None
        opt = T.get_optimizer(lin, kind, 1e-3, 0.9, ema_decay=0.99, ema_warmup=True)
        assert isinstance(opt.ema, ema.ShadowParams) and (opt.ema.decay, opt.ema.warmup) == (0.99, True)
        assert "ema" not in opt.state_dict() and list(opt.ema.state_dict()) == list(lin.state_dict())
    for kind, cls in (("Adam", torch.optim.Adam), ("sgd", torch.optim.SGD), ("RMSprop", torch.optim.RMSprop)):
        assert type(ae_train.get_optimizer(lin, kind, 1e-3)) is cls                       # unset: torch's own class, as before
        opt = ae_train.get_optimizer(lin, kind, 1e-3, ema_decay=0.5)
        assert isinstance(opt, cls) and isinstance(opt.ema, ema.ShadowParams) and opt._guard_opts is None
    for d in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            ema.ShadowParams(d)
    # the host restatement of the kernel's weight, and where the warm-up ends
    for decay, warm, t in ((0.5, False, 1), (0.9999, True, 1), (0.9999, True, 5), (0.999, True, 10 ** 6), (0.999, False, 3)):
        assert ema.weight(decay, warm, t) == float(kernel_w(decay, warm, t))
    n = ema.warmup_done(0.999)
    assert (1 + n) / (10 + n) >= float(np.float32(0.999)) > n / (9 + n)


def _bits(ts):
    return [t.detach().clone().view(torch.int32) for t in ts]


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_torchs_own_path_keeps_the_shadow(kind, guarded):
    """An nn.Linear has no engine: every step is torch's own, and the shadow follows in plain torch (host_update).  Six steps, the
    gradient of the fourth poisoned with an inf: the parameters are bit for bit those of a twin without EMA; the shadow is the
    float64 recurrence over the parameters after each step TAKEN, numbered by the steps taken; guarded, the skipped step leaves it
    bit for bit (unguarded, the inf goes into parameters and shadow alike, as it goes into the reference)."""
    from music_amd import train as T
    torch.manual_seed(0)
    a, b = torch.nn.Linear(5, 3), torch.nn.Linear(5, 3)
    b.load_state_dict(a.state_dict())
    gk = dict(max_grad_norm=0.1, skip_nonfinite=True) if guarded else {}
    decay, warm = 0.9, True
    opt = T.get_optimizer(a, kind, 1e-2, 0.9, ema_decay=decay, ema_warmup=warm, **gk)
    twin = T.get_optimizer(b, kind, 1e-2, 0.9, **gk)
    refs = [Ref64(p.detach().numpy()) for p in a.parameters()]                # taken at construction: the initial weights
    x = torch.randn(4, 5)
    taken = 0
    for step in range(6):
        for net in (a, b):
            net.zero_grad()
            net(x).pow(2).sum().backward()
            if step == 3:
                net.weight.grad[0, 0] = float("inf")
        before = _bits(opt.ema.state_dict().values())
        opt.step()
        twin.step()
        if guarded and step == 3:
            assert all(torch.equal(u, v) for u, v in zip(before, _bits(opt.ema.state_dict().values())))
            continue
        taken += 1
        for r, p in zip(refs, a.parameters()):
            r.step(p.detach().numpy(), kernel_w(decay, warm, taken))
    assert all(torch.equal(u, v) for u, v in zip(_bits(a.parameters()), _bits(b.parameters())))
    assert opt.ema.updates(opt._guard) == taken == (5 if guarded else 6)
    worst = max(r.check(s.numpy(), kind) for r, s in zip(refs, opt.ema.state_dict().values()))
    print(kind, "guarded" if guarded else "unguarded", "worst error / bound %.3g" % worst)
    if guarded:
        assert all(bool(torch.isfinite(s).all()) for s in opt.ema.state_dict().values())
        assert any(not torch.equal(s, p) for s, p in zip(opt.ema.state_dict().values(), a.parameters()))


class _Spec:
    total = 10
    off = {"a": 0, "b": 4}
    shape = {"a": (2, 2), "b": (6,)}


def _stub_engine():
    from music_amd.engine_base import EngineBase

    class Stub(EngineBase):
        def _make_workspace(self, B, T):
            return dict(B=B, T=T)
    eng = Stub()
    eng.device = torch.device("cpu")
    eng.flat, eng.flat_grad = torch.arange(10, dtype=torch.float32), torch.zeros(10)
    eng.spec, eng.param_names = _Spec(), ["a", "b"]
    eng._init_state()
    return eng


def test_engine_step_ends_with_the_one_launch(monkeypatch):
    """With _lib.call replaced (nothing is launched): adam_step issues wn_adam_flat then wn_ema_flat on a shadow that is a clone of the
    flat buffer, numbered by the host; the guarded step issues the guard, the guarded update and wn_ema_flat with the guard's state
    pointer and offset 0; unset, the step is what it was."""
    from music_amd import _lib
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(_lib, "stream", lambda: None)
    import music_amd.engine_base as eb
    monkeypatch.setattr(eb, "call", _lib.call)
    eng = _stub_engine()
    eng.adam_init(lr=1e-3)
    assert eng.ema is None
    eng.adam_step()
    assert [c[0] for c in calls] == ["wn_adam_flat"]
    eng.adam_init(lr=1e-3, ema_decay=0.999, ema_warmup=True)
    sh = eng.ema
    assert sh.flat is not eng.flat and torch.equal(sh.flat, eng.flat) and sh.flat.data_ptr() != eng.flat.data_ptr()
    assert [(n, tuple(t.shape), t.data_ptr() - sh.flat.data_ptr()) for n, t in sh.state_dict().items()] == [("a", (2, 2), 0), ("b", (6,), 16)]
    for t in (1, 2):
        del calls[:]
        eng.adam_step()
        assert [c[0] for c in calls] == ["wn_adam_flat", "wn_ema_flat"]
        assert calls[1][1] == (sh.flat.data_ptr(), eng.flat.data_ptr(), 10, 0.999, 1, t, None, None)
    eng.adam_init(lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.5)
    del calls[:]
    eng.adam_step(gscale=0.25)
    assert [c[0] for c in calls] == ["wn_grad_guard", "wn_adam_flat_guarded", "wn_ema_flat"]
    gd = eng.adam_state["guard"]
    assert calls[2][1] == (eng.ema.flat.data_ptr(), eng.flat.data_ptr(), 10, 0.5, 0, 0, gd.state_ptr(), None)
    # a restored run whose device counter starts elsewhere: the offset keeps T going
    gd.seed_taken(7)
    eng.ema.continue_from(12, 7)
    del calls[:]
    eng.adam_step()
    assert calls[2][1][5] == 5 and eng.ema.updates(gd) == 12


def test_swapped_holds_the_shadow_and_gives_everything_back():
    from music_amd import train as T
    torch.manual_seed(1)
    net = torch.nn.Linear(4, 2)
    opt = T.get_optimizer(net, "sgd", 0.1, 0.9, ema_decay=0.5)
    for _ in range(2):
        net.zero_grad()
        net(torch.randn(3, 4)).sum().backward()
        opt.step()
    params, shadow = _bits(net.parameters()), _bits(opt.ema.state_dict().values())
    assert any(not torch.equal(u, v) for u, v in zip(params, shadow))
    ids = [id(p) for p in net.parameters()]

    def unchanged():
        return (all(torch.equal(u, v) for u, v in zip(params, _bits(net.parameters()))) and
                all(torch.equal(u, v) for u, v in zip(shadow, _bits(opt.ema.state_dict().values()))))
    with opt.ema.swapped(net) as m:
        assert m is net and [id(p) for p in net.parameters()] == ids          # a content swap, not a rebind
        assert all(torch.equal(u, v) for u, v in zip(shadow, _bits(net.parameters())))
        with pytest.raises(RuntimeError, match="swapped"):
            opt.step()
        assert all(torch.equal(u, v) for u, v in zip(shadow, _bits(net.parameters())))
    assert unchanged()
    with pytest.raises(KeyError):
        with opt.ema.swapped(net):
            raise KeyError("from inside")
    assert unchanged()
    opt.step()                                                               # ... and steps are legal again
    # state_dict() / load_state_dict() round trip, also with a DataParallel prefix
    other = T.get_optimizer(torch.nn.Linear(4, 2), "sgd", 0.1, 0.9, ema_decay=0.5).ema
    other.load_state_dict({"module." + k: v for k, v in opt.ema.state_dict().items()}, n_updates=3)
    assert other.n_updates == 3 and all(torch.equal(u, v) for u, v in zip(other.state_dict().values(), opt.ema.state_dict().values()))


def test_rotation_removes_the_shadow_with_its_model(tmp_path):
    from music_amd import ae_train
    from music_amd import train as T
    d = str(tmp_path) + "/"
    for n in (3, 4):
        for suffix in (".model", ".opt", ".ema"):
            open(d + "wavenet%d%s" % (n, suffix), "w").close()
    T._rotate_checkpoints(d, 3)                                              # two stored: nothing goes (the .ema files are not counted)
    assert len(os.listdir(d)) == 6
    T._rotate_checkpoints(d, 2)
    assert sorted(os.listdir(d)) == ["wavenet4.ema", "wavenet4.model", "wavenet4.opt"]
    a = tmp_path / "ae"
    a.mkdir()
    for n in (9, 10):
        for suffix in (".model", ".ema"):
            open(str(a / ("wavenet_autoencoder%d%s" % (n, suffix))), "w").close()
    import glob
    ae_train._rotate_checkpoints(glob.glob(str(a) + "/*.model"), 2)
    assert sorted(os.listdir(a)) == ["wavenet_autoencoder10.ema", "wavenet_autoencoder10.model"]


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_a_restored_optimizer_continues_the_count(kind, guarded, tmp_path):
    """What train() does at a checkpoint and at a resume, on torch's own path: the optimizer's state_dict, the shadow (save_shadow) and
    the count of updates are saved after 3 steps; a new optimizer and shadow restored from them take 3 more - the shadow equals that
    of 6 steps straight bit for bit (the warm-up is on: T has to continue; SGD's guard restarts its device count at 1)."""
    from music_amd import ema
    from music_amd import train as T
    gk = dict(max_grad_norm=0.1, skip_nonfinite=True) if guarded else {}
    torch.manual_seed(2)
    xs = [torch.randn(4, 5) for _ in range(6)]

    def steps(net, opt, batches):
        for x in batches:
            net.zero_grad()
            net(x).pow(2).sum().backward()
            opt.step()
    torch.manual_seed(3)
    a = torch.nn.Linear(5, 3)
    init = {k: v.clone() for k, v in a.state_dict().items()}
    oa = T.get_optimizer(a, kind, 1e-2, 0.9, ema_decay=0.9, ema_warmup=True, **gk)
    steps(a, oa, xs)
    b = torch.nn.Linear(5, 3)
    b.load_state_dict(init)
    ob = T.get_optimizer(b, kind, 1e-2, 0.9, ema_decay=0.9, ema_warmup=True, **gk)
    steps(b, ob, xs[:3])
    ema.save_shadow(ob.ema, str(tmp_path / "wavenet1.ema"))
    saved = dict(model={k: v.clone() for k, v in b.state_dict().items()}, opt=ob.state_dict(), n=ob.ema.updates(ob._guard))
    assert saved["n"] == 3
    c = torch.nn.Linear(5, 3)
    c.load_state_dict(saved["model"])
    oc = T.get_optimizer(c, kind, 1e-2, 0.9, ema_decay=0.9, ema_warmup=True, **gk)
    oc.load_state_dict(saved["opt"])
    ema.restore_shadow(oc.ema, str(tmp_path / "wavenet1.ema"), saved["n"], oc._guard)
    steps(c, oc, xs[3:])
    assert oc.ema.updates(oc._guard) == 6 == oa.ema.updates(oa._guard)
    for u, v in zip(_bits(oa.ema.state_dict().values()), _bits(oc.ema.state_dict().values())):
        assert torch.equal(u, v)
    # no saved count: the warm-up counts as finished; no file: the shadow stays the restored weights, and one line says so
    od = T.get_optimizer(c, kind, 1e-2, 0.9, ema_decay=0.9, ema_warmup=True, **gk)
    ema.restore_shadow(od.ema, str(tmp_path / "none.ema"), None, None)
    assert ema.weight(0.9, True, od.ema.n_updates + 1) == ema.weight(0.9, False, 1)
    assert all(torch.equal(s, p) for s, p in zip(od.ema.state_dict().values(), c.parameters()))
