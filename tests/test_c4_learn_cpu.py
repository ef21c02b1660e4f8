"""Host side of the Connect4 weight refresh and spai.learn: the two new entry
points are declared, exported and bound with the declared signatures, NULL
arguments are refused without a device, and spai.learn refuses a bad `refresh`
or `dtype` before it creates an engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

DECLS = {
    "spai_net_set_params": r"int spai_net_set_params\(spai_net \*net, const float \*params, size_t n_params\);",
    "spai_net_set_params_from_learner": r"int spai_net_set_params_from_learner\(spai_net \*net, spai_learner \*l\);",
}


@pytest.fixture(scope="module")
def spai():
    import spai as s
    s.lib()
    return s


def test_symbols_and_signatures(spai):
    with open(os.path.join(REPO, "include", "spai.h")) as f:
        hdr = f.read()
    L = spai.lib()
    for name, decl in DECLS.items():
        assert len(re.findall(decl, hdr)) == 1, name
        assert spai.SYMBOLS.count(name) == 1 and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert L.spai_net_set_params.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t]
    assert L.spai_net_set_params_from_learner.argtypes == [C.c_void_p, C.c_void_p]
    with open(os.path.join(REPO, "rust", "src", "spai_sys.rs")) as f:
        rs = f.read()
    for name in DECLS:
        assert len(re.findall(r"pub fn %s\(" % name, rs)) == 1, name
    assert callable(spai.Net.set_params) and callable(spai.learn)


def test_null_arguments(spai):
    L = spai.lib()
    p = np.zeros(spai.num_params(1), np.float32)
    assert L.spai_net_set_params(None, p.ctypes.data_as(C.c_void_p), p.size) == -1
    assert b"NULL" in L.spai_last_error()
    assert L.spai_net_set_params_from_learner(None, None) == -1
    assert b"NULL" in L.spai_last_error()


class _NoEngine(Exception):
    pass


@pytest.mark.parametrize("kw", [dict(refresh="nonsense"), dict(refresh=None), dict(dtype=7), dict(dtype="bf16")])
def test_learn_refuses_bad_arguments_before_a_device(spai, monkeypatch, tmp_path, kw):
    def no_engine(*a, **k):
        raise _NoEngine("spai.learn created an engine")
    monkeypatch.setattr(spai, "Engine", no_engine)
    with pytest.raises(ValueError):
        spai.learn(num_learn_iters=1, num_self_play_iters=1, num_parallel_self_play_games=2, num_searches=2,
                   blocks=0, checkpoint_dir=str(tmp_path), **kw)
    assert not os.listdir(tmp_path)


def test_learn_good_arguments_reach_the_engine(spai, monkeypatch, tmp_path):
    """the same call with a valid refresh and dtype goes on to create its engine"""
    def no_engine(*a, **k):
        raise _NoEngine
    monkeypatch.setattr(spai, "Engine", no_engine)
    for kw in (dict(), dict(refresh="host", dtype=spai.DTYPE_F32), dict(refresh="device", dtype=spai.DTYPE_BF16)):
        with pytest.raises(_NoEngine):
            spai.learn(num_learn_iters=1, num_self_play_iters=1, num_parallel_self_play_games=2, num_searches=2,
                       blocks=0, checkpoint_dir=str(tmp_path), **kw)
