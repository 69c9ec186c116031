"""The path limiter's call in the header, the ctypes table and the built library, every refusal it makes before anything is launched --
invalid-argument status with the call's name in mf_last_error() --, and the Python refusals of `ops.path_limit` and of the session's keywords.
Host addresses throughout: a call that got as far as a launch would not return MF_ERR_INVALID_ARG.  No GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'mf_path_limit_f64'
N, R, C, W, H = 3, 2, 3, 128, 96
S = (R + 1) * (C + 1) * 2


def test_library_exports_the_call():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 19 and hasattr(_lib.lib, NAME)
    assert _lib.SIGNATURES[NAME][1][11] is ctypes.c_double
    assert re.search(r'\bint %s\(' % NAME, header)
    block = header[header.index('---- path limit'):header.index('int %s(' % NAME)]
    for text in ('tests/path_limit_model.py', 'No atomics', 'Asynchronous on `stream`', 'no fma', 'MF_ERR_INVALID_ARG, nothing launched', 'never waits',
                 'a < b ? a : b', 'Interior vertices play no part', 'candidate 0 is never tested', 'bit for bit when k_t == K', 'clamped to 0 .. K',
                 'row 0 from column 0 to C-1', 'd_k_prev is null'):
        assert text in block, text
    for name, value in (('MF_PATH_LIMIT_MAX_STEPS', _lib.PATH_LIMIT_MAX_STEPS), ('MF_PATH_LIMIT_MAX_BOUNDARY', _lib.PATH_LIMIT_MAX_BOUNDARY)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name
    assert (_lib.PATH_LIMIT_MAX_STEPS, _lib.PATH_LIMIT_MAX_BOUNDARY) == (64, 1024)
    makefile = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'Makefile')).read()
    assert ' path_limit.hip' in makefile and 'path_limit_body.h' in makefile


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (8 * 4096 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, *args):
    rc = getattr(_lib.lib, NAME)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (args, rc, err)
    assert NAME.encode() + b':' in err, err
    return err


def test_c_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    # 4 KB apart: a path is N * S * 8 = 576 bytes, k_raw and k 12, k_prev 4
    keys = ('unstab', 'stab', 'k_prev', 'k_raw', 'k', 'out')
    at = {key: base + 4096 * i for i, key in enumerate(keys)}
    good = dict(n=N, W=W, H=H, R=R, C=C, rect=(10, 7, 117, 88), guard=2.0, steps=32, rise=2, **at)
    path = N * S * 8

    def call(**kw):
        a = dict(good, **kw)
        return (vp(a['unstab']), vp(a['stab']), a['n'], a['W'], a['H'], a['R'], a['C'], *a['rect'], a['guard'], a['steps'], a['rise'], vp(a['k_prev']),
                vp(a['k_raw']), vp(a['k']), vp(a['out']), None)

    for n in (0, -1):
        assert b'n must be at least 1' in refused(_lib, *call(n=n)), n
    for kw in (dict(R=0), dict(C=0), dict(R=-1), dict(R=256, C=257), dict(R=1, C=512), dict(R=1 << 30, C=1 << 30)):
        assert b'boundary vertices' in refused(_lib, *call(**kw)), kw
    for kw in (dict(W=1), dict(H=1), dict(W=0), dict(H=-5)):
        assert b'W and H must be at least 2' in refused(_lib, *call(**kw)), kw
    for rect in ((-1, 7, 117, 88), (10, -1, 117, 88), (118, 7, 117, 88), (10, 89, 117, 88), (10, 7, 128, 88), (10, 7, 117, 96)):
        assert b'is not inside a 128 x 96 frame' in refused(_lib, *call(rect=rect)), rect
    for steps in (0, -1, 65, 1 << 20):
        assert b'steps must be in 1 .. 64' in refused(_lib, *call(steps=steps)), steps
    for kw in (dict(rise=0), dict(rise=-1), dict(rise=33), dict(steps=1, rise=2)):
        assert b'rise must be in 1 .. steps' in refused(_lib, *call(**kw)), kw
    for guard in (-1.0, -1e-300, float('inf'), float('-inf'), float('nan')):
        assert b'guard must be finite and >= 0' in refused(_lib, *call(guard=guard)), guard
    for key in keys:
        if key != 'k_prev':
            assert b'null' in refused(_lib, *call(**{key: None})), key
    for key in keys:
        assert b'aligned' in refused(_lib, *call(**{key: at[key] + (2 if key in ('k_prev', 'k_raw', 'k') else 4)})), key
    # an output over an input: first and last byte; over the carried word
    for kw in (dict(out=at['unstab']), dict(out=at['stab'] + path - 8), dict(out=at['unstab'] - path + 8), dict(k=at['stab'] + path - 4), dict(k_raw=at['unstab']),
               dict(k_prev=at['out'] + path - 4), dict(k_prev=at['k']), dict(k_prev=at['k_raw'] + 8)):
        assert b'an output aliases an input' in refused(_lib, *call(**kw)), kw
    for kw in (dict(k=at['k_raw']), dict(k=at['k_raw'] + 8), dict(k_raw=at['out'] + path - 4), dict(k=at['out'])):
        assert b'two of the outputs alias' in refused(_lib, *call(**kw)), kw
    # the limits themselves are accepted as far as the checks go: next to a refusal that comes last
    for kw in (dict(R=256, C=256), dict(R=1, C=511), dict(steps=64, rise=64), dict(steps=1, rise=1), dict(guard=0.0), dict(rect=(0, 0, 127, 95)),
               dict(rect=(5, 5, 5, 5)), dict(W=2, H=2, rect=(0, 0, 1, 1)), dict(k_prev=None)):
        assert b'alias' in refused(_lib, *call(**dict(kw, k=at['k_raw']))), kw                  # (a 256 x 256 path is 3 MB: it reaches the inputs too)
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    c = torch.zeros((N, S), dtype=torch.float64)
    rect = (10, 7, 117, 88)
    assert (ops.PATH_LIMIT_STEPS, ops.PATH_LIMIT_GUARD, ops.PATH_LIMIT_RISE) == (32, 2.0, 2)
    for kw, match in ((dict(R=0), 'the mesh needs'), (dict(R=256, C=257), 'the mesh needs'), (dict(W=1), 'W and H must be at least 2'),
                      (dict(rectangle=(10, 7, 128, 88)), 'is not inside a 128 x 96 frame'), (dict(rectangle=(11, 7, 10, 88)), 'is not inside'),
                      (dict(rectangle=(10, 7, 117)), r'rectangle must be \(left, top, right, bottom\)'), (dict(rectangle=None), 'rectangle must be'),
                      (dict(steps=0), 'steps must be an integer in 1 .. 64'), (dict(steps=65), 'steps must be'), (dict(steps=32.0), 'steps must be'),
                      (dict(steps=True), 'steps must be'), (dict(rise=0), 'rise must be an integer in 1 .. steps = 32'), (dict(rise=33), 'rise must be'),
                      (dict(steps=4, rise=5), 'rise must be an integer in 1 .. steps = 4'), (dict(guard=-0.5), 'guard must be a finite number >= 0'),
                      (dict(guard=float('nan')), 'guard must be'), (dict(guard=float('inf')), 'guard must be'), (dict(guard='2'), 'guard must be')):
        a = dict(dict(W=W, H=H, R=R, C=C, rectangle=rect), **kw)
        with pytest.raises(ValueError, match=match):
            ops.path_limit(c, c, **a)
    # the tensors come after the numbers: a host tensor gets as far as this
    with pytest.raises(ValueError, match='unstab must be a CUDA/HIP'):
        ops.path_limit(c, c, W, H, R, C, rect)
    with pytest.raises(ValueError, match='unstab must be a CUDA/HIP'):
        ops.path_limit(c.numpy(), c, W, H, R, C, rect)
    assert ops.check_path_limit(64, 0, 64) == (64, 0.0, 64) and ops.check_path_limit(1, 2.5, 1) == (1, 2.5, 1)


def test_session_keyword_refusals():
    pytest.importorskip('torch')
    from meshflow_amd import online

    class Stub:                                                          # what OnlineSession reads before its own checks are through
        temporal_smoothing_radius = 2

        def _check_definition(self, definition):
            pass

    for kw, match in ((dict(on_uncovered='crop'), "on_uncovered must be 'report' or 'limit'"), (dict(on_uncovered=None), 'on_uncovered must be'),
                      (dict(limit_steps=0), 'limit_steps must be an integer in 1 .. 64'), (dict(limit_steps=65), 'limit_steps must be'),
                      (dict(limit_rise=0), 'limit_rise must be an integer in 1 .. limit_steps = 32'), (dict(limit_rise=33), 'limit_rise must be'),
                      (dict(limit_steps=8, limit_rise=9), 'limit_rise must be an integer in 1 .. limit_steps = 8'),
                      (dict(limit_guard=-1.0), 'limit_guard must be a finite number >= 0'), (dict(limit_guard=float('nan')), 'limit_guard must be'),
                      (dict(limit_guard=float('inf')), 'limit_guard must be')):
        with pytest.raises(ValueError, match=match):
            online.OnlineSession(Stub(), **kw)
    # with 'limit', a rectangle the guard does not fit around: refused from the shape alone, before anything touches a device
    session = online.OnlineSession.__new__(online.OnlineSession)
    session.crop_margin, session.limit_guard = 0.02, 2.0

    class Frames:
        shape = (2, 96, 128)

    with pytest.raises(ValueError, match='widen crop_margin'):
        session._check_limit_fits(Frames())
    with pytest.raises(ValueError, match='widen crop_margin'):
        session._check_limit_fits((Frames(), Frames()))                  # (a 4:2:0 pair)
    session.crop_margin = 0.08
    session._check_limit_fits(Frames())                                  # 10 columns, 7 rows: room for the guard and a pixel
    session.limit_guard = 6.5
    with pytest.raises(ValueError, match='limit_guard=6.5 needs 7.5'):
        session._check_limit_fits(Frames())
