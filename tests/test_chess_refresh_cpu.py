"""Host side of the chess weight refresh and spai_chess.learn's `refresh`: the two
new entry points are declared, exported and bound with the declared signatures,
NULL arguments are refused without a device, and spai_chess.learn refuses a bad
`refresh` before it creates an engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

DECLS = {
    "spai_chess_net_set_params_from_learner":
        r"int spai_chess_net_set_params_from_learner\(spai_chess_net \*net, spai_chess_learner \*l\);",
    "spai_chess_net_image": r"int spai_chess_net_image\(spai_chess_net \*net, void \*out, size_t cap, size_t \*bytes\);",
}


@pytest.fixture(scope="module")
def sc():
    import spai_chess as s
    s.lib()
    return s


def test_symbols_and_signatures(sc):
    import spai
    with open(os.path.join(REPO, "include", "spai.h")) as f:
        hdr = f.read()
    L = sc.lib()
    for name, decl in DECLS.items():
        assert len(re.findall(decl, hdr)) == 1, name
        assert spai.SYMBOLS.count(name) == 1 and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    assert L.spai_chess_net_set_params.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t]
    assert L.spai_chess_net_set_params_from_learner.argtypes == [C.c_void_p, C.c_void_p]
    assert L.spai_chess_net_image.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    with open(os.path.join(REPO, "rust", "src", "spai_sys.rs")) as f:
        rs = f.read()
    for name in list(DECLS) + ["spai_chess_net_set_params"]:
        assert len(re.findall(r"pub fn %s\(" % name, rs)) == 1, name
    assert callable(sc.ChessNet.set_params) and callable(sc.ChessNet.image) and callable(sc.learn)


def test_null_arguments(sc):
    L = sc.lib()
    n = C.c_size_t()
    buf = np.zeros(16, np.uint8)
    assert L.spai_chess_net_set_params_from_learner(None, None) == -1
    assert b"NULL" in L.spai_last_error()
    assert L.spai_chess_net_image(None, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == -1
    assert b"NULL" in L.spai_last_error()
    assert L.spai_chess_net_image(None, None, 0, None) == -1
    assert b"NULL" in L.spai_last_error()


class _NoEngine(Exception):
    pass


@pytest.mark.parametrize("kw", [dict(refresh="nonsense"), dict(refresh=None)])
def test_learn_refuses_a_bad_refresh_before_a_device(sc, monkeypatch, tmp_path, kw):
    def no_engine(*a, **k):
        raise _NoEngine("spai_chess.learn created an engine")
    monkeypatch.setattr(sc, "ChessEngine", no_engine)
    with pytest.raises(ValueError):
        sc.learn(num_learn_iters=1, num_self_play_iters=1, num_parallel_self_play_games=2, num_searches=2, blocks=0,
                 checkpoint_dir=str(tmp_path), **kw)
    assert not os.listdir(tmp_path)


def test_learn_good_refresh_reaches_the_engine(sc, monkeypatch, tmp_path):
    """the same call with a valid refresh goes on to create its engine"""
    def no_engine(*a, **k):
        raise _NoEngine
    monkeypatch.setattr(sc, "ChessEngine", no_engine)
    for kw in (dict(), dict(refresh="host"), dict(refresh="device")):
        with pytest.raises(_NoEngine):
            sc.learn(num_learn_iters=1, num_self_play_iters=1, num_parallel_self_play_games=2, num_searches=2,
                     blocks=0, checkpoint_dir=str(tmp_path), **kw)
