"""mmg_sup_draw_select without a GPU: the refusals that come before any HIP call, and the binding ops.py derives from the
header's prototype."""
import ctypes


def test_refusals_come_before_any_launch():
    import mmgnn  # noqa: F401
    from mmgnn import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)                     # never touched
    n = 5000
    need = lib.mmg_sup_draw_select_ws_bytes(n)
    assert need >= 1024 * 8 + ((n + 2047) // 2048) * 256 * 2 and lib.mmg_sup_draw_select_ws_bytes(-1) == 0
    assert lib.mmg_sup_draw_select_ws_bytes(0) > 0

    def call(fraction=0.2, n_pairs=n, max_groups=0, counts=p, pi=p, ws=p, ws_bytes=need):
        rc = lib.mmg_sup_draw_select(None, 1, fraction, None, None, pi, p, 20, n_pairs, max_groups, p, p, p, counts, p, p,
                                     ws, ws_bytes, None)
        return rc, lib.mmg_last_error()

    rc, msg = call(ws_bytes=need - 1)
    assert rc == -3 and b"sup_draw_select" in msg and b"workspace" in msg
    rc, msg = call(ws=None)
    assert rc == -3 and b"sup_draw_select" in msg and b"workspace" in msg
    for bad in (dict(fraction=-0.1), dict(fraction=1.5), dict(n_pairs=-1), dict(n_pairs=2 ** 31), dict(max_groups=-1),
                dict(max_groups=1025), dict(counts=None), dict(pi=None)):
        rc, msg = call(**bad)
        assert rc == -1 and b"sup_draw_select" in msg, bad


def test_the_prototype_is_bound_from_the_header():
    import mmgnn  # noqa: F401
    from mmgnn import _lib, ops
    names = [q[0] for q in _lib.PARAMS["mmg_sup_draw_select"]]
    assert names == ["seed_ptr", "seed", "fraction", "ids", "io_perm", "pi", "deg", "degree_threshold", "n_pairs",
                     "max_groups", "sup", "sel_low", "sel_high", "counts", "count", "inv_den", "ws", "ws_bytes", "stream"]
    plan, n_given = ops._PLANS["mmg_sup_draw_select"]
    assert n_given == 16 and plan[-3:] == ["ws", "ws_bytes", "stream"]
