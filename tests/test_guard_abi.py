"""CPU checks of the ABI 9 entry points of the guarded optimizer step (wn_grad_guard, wn_adam_flat_guarded, wn_sgd_flat_guarded,
wn_rmsprop_flat_guarded; include/wavenet_hip.h) and of its host surface (music_amd/guard.py): declared, exported, bound, NULL
pointers refused by name before anything is launched, the JSON keys, the guard_log.log line.  No device is touched."""
import ctypes
import os
import re

import pytest
import torch

from tests.helpers import ROOT

NEW = ["wn_grad_guard", "wn_adam_flat_guarded", "wn_sgd_flat_guarded", "wn_rmsprop_flat_guarded"]


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


def test_abi_version_is_9_everywhere():
    from music_amd import _lib
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", _header()).group(1)) == 9
    assert _lib.ABI_VERSION == 9
    assert _lib.load().wn_version() == 9


def test_new_names_are_declared_exported_and_bound():
    from music_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    # argument counts of the declarations and of the ctypes table agree
    for name in NEW:
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name


def test_state_struct_has_the_documented_size_and_layout():
    from music_amd import _lib
    src = _header()
    nbytes = int(re.search(r"#define WN_GUARD_STATE_BYTES (\d+)", src).group(1))
    assert ctypes.sizeof(_lib.GuardState) == nbytes == 48
    assert int(re.search(r"#define WN_GUARD_NUM_PARTIALS (\d+)", src).group(1)) == _lib.GUARD_NUM_PARTIALS == 256
    assert re.search(r"#define WN_GUARD_PARTIALS_BYTES \(WN_GUARD_NUM_PARTIALS \* 12\)", src)
    assert _lib.GUARD_PARTIALS_BYTES == 256 * 12
    # the member order of the C struct is the ctypes one
    body = re.search(r"typedef struct wn_guard_state \{(.*?)\} wn_guard_state;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\b(float|uint32_t|uint64_t)\s+(\w+);", body)
    ctype = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    assert [(n, ctype[t]) for t, n in members] == list(_lib.GuardState._fields_)
    assert _lib.GuardState.n_taken.offset == 16 and _lib.GuardState.bc1.offset == 40


def test_null_pointers_are_refused_by_name_and_empty_calls_pass():
    from music_amd import _lib
    lib = _lib.load()
    P = 1 << 20            # "some non-NULL address": never dereferenced, every case below is refused (or empty) before a launch

    def bad(name, arg, *args):
        rc = getattr(lib, name)(*args)
        msg = lib.wn_last_error().decode()
        assert rc == -4 and name in msg and ("'%s'" % arg) in msg, (name, rc, msg)

    #        g  n  gscale max_norm skip b1 b2 partials state stream
    guard = [P, 8, 1.0, 1.0, 1, 0.9, 0.999, P, P, None]
    for i, arg in ((0, "g"), (7, "partials"), (8, "state")):
        a = list(guard)
        a[i] = None
        bad("wn_grad_guard", arg, *a)
    a = list(guard)
    a[1], a[7] = 0, None                                   # an empty gradient still needs the partials and the state block
    bad("wn_grad_guard", "partials", *a)
    assert lib.wn_grad_guard(P, -1, 1.0, 1.0, 1, 0.9, 0.999, P, P, None) == -4
    assert lib.wn_grad_guard(P + 2, 8, 1.0, 1.0, 1, 0.9, 0.999, P, P, None) == -4 and b"align" in lib.wn_last_error()
    #       p  g  m  v  n  lr   b1   b2     eps  gscale state stream
    adam = [P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 1.0, P, None]
    for i, arg in ((0, "p"), (1, "g"), (2, "m"), (3, "v"), (10, "state")):
        a = list(adam)
        a[i] = None
        bad("wn_adam_flat_guarded", arg, *a)
    #      p  g  buf n  lr  mom gscale state stream
    sgd = [P, P, P, 8, 0.1, 0.9, 1.0, P, None]
    for i, arg in ((0, "p"), (1, "g"), (7, "state")):
        a = list(sgd)
        a[i] = None
        bad("wn_sgd_flat_guarded", arg, *a)
    assert lib.wn_sgd_flat_guarded(P, P, None, 8, 0.1, 0.9, 1.0, P, None) == -4 and b"wn_sgd_flat_guarded" in lib.wn_last_error()
    #      p  g  sq buf n  lr  alpha eps  mom gscale state stream
    rms = [P, P, P, P, 8, 0.1, 0.99, 1e-8, 0.9, 1.0, P, None]
    for i, arg in ((0, "p"), (1, "g"), (10, "state")):
        a = list(rms)
        a[i] = None
        bad("wn_rmsprop_flat_guarded", arg, *a)
    assert lib.wn_rmsprop_flat_guarded(P, P, None, None, 8, 0.1, 0.99, 1e-8, 0.0, 1.0, P, None) == -4
    assert b"wn_rmsprop_flat_guarded" in lib.wn_last_error()
    # n == 0: nothing to update, NULLs allowed, status 0 (wn_grad_guard with n == 0 still launches its finalizer: tests/test_gpu_guard.py)
    assert lib.wn_adam_flat_guarded(None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None) == 0
    assert lib.wn_sgd_flat_guarded(None, None, None, 0, 0.1, 0.0, 1.0, None, None) == 0
    assert lib.wn_rmsprop_flat_guarded(None, None, P, None, 0, 0.1, 0.99, 1e-8, 0.0, 1.0, None, None) == 0


def test_json_keys_and_optimizer_options():
    from music_amd import ae_train, guard
    from music_amd import train as T
    assert guard.guard_options({}) == (None, False)
    assert guard.guard_options({"max_grad_norm": 2, "skip_nonfinite": True}) == (2.0, True)
    assert guard.guard_options({"skip_nonfinite": 1}) == (None, True)
    assert not guard.enabled(None, False) and guard.enabled(0.5, False) and guard.enabled(None, True)
    lin = torch.nn.Linear(3, 2)
    for kind, cls in (("adam", torch.optim.Adam), ("sgd", torch.optim.SGD), ("rmsprop", torch.optim.RMSprop)):
        plain = T.get_optimizer(lin, kind, 1e-3, 0.9)
        opt = T.get_optimizer(lin, kind, 1e-3, 0.9, max_grad_norm=1.0, skip_nonfinite=True)
        assert isinstance(opt, cls) and plain._guard_opts is None and opt._guard_opts == (1.0, True)
        assert plain.guard_report() is None
    for kind, cls in (("Adam", torch.optim.Adam), ("sgd", torch.optim.SGD), ("RMSprop", torch.optim.RMSprop)):
        assert type(ae_train.get_optimizer(lin, kind, 1e-3)) is cls                       # unset: torch's own class, as before
        assert isinstance(ae_train.get_optimizer(lin, kind, 1e-3, max_grad_norm=1.0), cls)
    with pytest.raises(ValueError):
        ae_train.get_optimizer(lin, "lbfgs", 1e-3, skip_nonfinite=True)


@pytest.mark.parametrize("kind", ["adam", "sgd", "rmsprop"])
def test_host_rule_of_a_step_on_torchs_own_path(kind):
    """A module without an engine steps on torch's own path; the guard's rule is applied on the host: clip_grad_norm_ first, and a
    non-finite gradient is not applied, does not count as a step, and leaves parameters and state as they were."""
    from music_amd import train as T
    torch.manual_seed(0)
    a, b = torch.nn.Linear(5, 3), torch.nn.Linear(5, 3)
    b.load_state_dict(a.state_dict())
    opt = T.get_optimizer(a, kind, 1e-2, 0.9, max_grad_norm=0.1, skip_nonfinite=True)
    ref = {"adam": lambda: torch.optim.Adam(b.parameters(), lr=1e-2), "sgd": lambda: torch.optim.SGD(b.parameters(), lr=1e-2, momentum=0.9),
           "rmsprop": lambda: torch.optim.RMSprop(b.parameters(), lr=1e-2, momentum=0.9)}[kind]()
    x = torch.randn(4, 5)
    for step in range(4):
        for net in (a, b):
            net.zero_grad()
            net(x).pow(2).sum().backward()
        if step == 1:
            before = [p.detach().clone() for p in a.parameters()]
            a.weight.grad[0, 0] = float("inf")
            opt.step()
            assert all(torch.equal(p, q) for p, q in zip(a.parameters(), before))
            continue                                        # the reference simply omits this step
        torch.nn.utils.clip_grad_norm_(b.parameters(), 0.1)
        opt.step()
        ref.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.allclose(p, q, rtol=0, atol=1e-7)
    rep = opt.guard_report()
    assert (rep["taken"], rep["skipped"], rep["clipped"]) == (3, 1, 3)
    if kind != "sgd":
        assert float(opt.state_dict()["state"][0]["step"]) == 3.0


def test_guard_log_line_and_warning(tmp_path, capsys):
    from music_amd import guard
    reports = [dict(norm=1.5, coef=0.5, taken=10, clipped=4, skipped=0, nonfinite=0),
               dict(norm=float("inf"), coef=float("nan"), taken=18, clipped=5, skipped=2, nonfinite=7),
               dict(norm=0.25, coef=1.0, taken=27, clipped=5, skipped=3, nonfinite=0)]
    it = iter(reports)
    grads = [("causal_layer.weight", torch.tensor([1.0, float("nan")])), ("post.bias", torch.ones(3)), ("unused", None)]
    log = guard.GuardLog(str(tmp_path / "guard_log.log"), lambda: next(it), lambda: grads)
    for n in (10, 20, 30):
        log.tick(n)
    lines = open(tmp_path / "guard_log.log").read().splitlines()
    assert lines == ["Trained over 10 pieces,Gradient norm is 1.5,clipped 4,skipped 0",
                     "Trained over 20 pieces,Gradient norm is inf,clipped 1,skipped 2",
                     "Trained over 30 pieces,Gradient norm is 0.25,clipped 0,skipped 1"]
    assert int(lines[-1].split(' ')[2]) == 30                  # third word = pieces trained, as in loss_log.log
    err = capsys.readouterr().err
    assert err.count("was skipped") == 1                       # one warning, the first time the count grows
    assert "causal_layer.weight" in err and "post.bias" not in err and guard.BF16_HINT in err
    # no guard yet (no step taken): nothing is written
    quiet = guard.GuardLog(str(tmp_path / "none.log"), lambda: None, lambda: [])
    assert quiet.tick(5) is None and not os.path.exists(tmp_path / "none.log")


def test_train_wires_the_keys_with_the_launches_patched_out(monkeypatch):
    """The fused step's options reach the engine, and the guarded step calls wn_grad_guard then wn_adam_flat_guarded (never the plain
    entry) - with _lib.call replaced, on CPU tensors, so nothing is launched."""
    from music_amd import _lib, guard

    class Eng:
        pass
    eng = Eng()
    eng.flat, eng.flat_grad = torch.zeros(10), torch.zeros(10)
    eng.spec = type("S", (), {"total": 10, "off": {"a": 0, "b": 4}, "shape": {"a": (2, 2), "b": (6,)}})()
    eng.param_names = ["a", "b"]
    eng.adam_state = guard.adam_init_guard(dict(m=torch.zeros(10), v=torch.zeros(10), t=0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8),
                                           "cpu", 0.5, True)
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(_lib, "stream", lambda: None)
    guard.adam_step_guarded(eng, 0.25)
    assert [c[0] for c in calls] == ["wn_grad_guard", "wn_adam_flat_guarded"]
    g = calls[0][1]
    assert g[1] == 10 and g[2] == 0.25 and g[3] == 0.5 and g[4] == 1 and (g[5], g[6]) == (0.9, 0.999)
    assert calls[1][1][-2] == g[8]                              # the update reads the state block the guard wrote
    assert [(n, v.numel()) for n, v in guard.engine_named_grads(eng)] == [("a", 4), ("b", 6)]
    gd = eng.adam_state["guard"]
    gd.seed_taken(7)
    assert guard.engine_guard_report(eng)["taken"] == 7 and eng.adam_state["t"] == 7
    assert guard.adam_init_guard(dict(b1=0.9, b2=0.999), "cpu", None, False)["guard"] is None
