"""CPU-only: the routes of the conv kernel x mode matrix (tests/conv_matrix_cases.py).  tests/test_hip_conv_matrix.py runs every launch
of that table on the GPU and means a NAMED kernel by each; here the library's host-only query es_conv_kernel_of answers, for the
same arguments under the same route options, which kernel es_conv_mfma_f16 would launch and how it would split K -- so a change of
the routing rule that moves a case onto another kernel fails here, without a GPU, instead of leaving a kernel untested.  Also: the
table reaches every kernel conv_launch() can launch, and every kernel with mode handling in all six modes.  No device compute."""
import ctypes as C
import os

import numpy as np
import pytest

import conv_matrix_cases as cm
from conftest import GOLDEN
from test_conv_route_cpu import _conv_args, _options, _set


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def _kernel_of(L, a):
    name = C.create_string_buffer(32)
    S = L.es_conv_kernel_of(C.byref(a), name, 32)
    return name.value.decode(), S


def test_every_launch_of_the_matrix_takes_the_kernel_the_table_names(L):
    found = _options(L)
    bad, n = [], 0
    try:
        for case in cm.CASES:
            for r in case['routes']:
                _set(L, found)
                _set(L, r.options.items())
                got = _kernel_of(L, cm.dummy_conv_args(case, r.splitk))
                n += 1
                if got != (cm.expected_kernel(r.kernel), r.S):
                    bad.append('%s [%s]: %s, S = %d; the table says %s, S = %d' % ((case['name'], cm.route_label(r)) + got + (r.kernel, r.S)))
    finally:
        _set(L, found)
    assert n >= 380 and not bad, '%d of %d routes differ:\n%s' % (len(bad), n, '\n'.join(bad))


def test_the_matrix_reaches_every_kernel_and_every_mode_of_the_kernels_that_handle_modes():
    reached = {}
    for case in cm.CASES:
        for r in case['routes']:
            reached.setdefault(r.kernel, set()).add(case['mode'])
    assert set(reached) == set(cm.KERNELS), 'not reached / unknown: %s' % sorted(set(reached) ^ set(cm.KERNELS))
    for k in cm.MODE_KERNELS:
        assert reached[k] == set(range(6)), '%s is reached in modes %s only' % (k, sorted(cm.MODE_NAMES[m] for m in reached[k]))
    for fam in 'AB':                   # both families, every mode, and the skip phase wherever a mode takes one
        have = {(c['mode'], bool(c['Cin2'])) for c in cm.FAMILY_CASES if c['family'] == fam}
        assert have == {(m, s) for m in range(6) for s in (False, True) if not (s and m in cm.UP_MODES)}
    labels = [c['name'] for c in cm.CASES]
    assert len(set(labels)) == len(labels)


def test_the_kernel_names_are_the_enumerators_of_the_library(L):
    """the forcing options name every tile; a name the library does not know would never compare equal"""
    found = _options(L)
    case = cm.FAMILY_CASES[0]
    try:
        _set(L, [('conv_st_bm', 128), ('conv_st_np', 8), ('conv_st_ns', 6)])          # not a built tile
        assert _kernel_of(L, cm.dummy_conv_args(case, None)) == ('none', 1)
    finally:
        _set(L, found)
    a = cm.dummy_conv_args(case, None)
    assert L.es_conv_kernel_of(C.byref(a), None, 0) == 2                              # (no name wanted: the split alone)
    short = C.create_string_buffer(b'xxxxxxxx', 8)
    assert L.es_conv_kernel_of(C.byref(a), short, 5) == 2 and short.raw[:5] == b'ws_1\0' and short.raw[5:] == b'xxx'


def test_invalid_arguments_and_the_up_modes_with_a_skip_are_refused(L):
    a = cm.dummy_conv_args(cm.FAMILY_CASES[0], None)
    a.taps = 5
    name = C.create_string_buffer(b'untouched', 32)
    assert L.es_conv_kernel_of(C.byref(a), name, 32) == -1 and b'taps' in L.es_last_error() and name.value == b'untouched'
    for mode in cm.UP_MODES:
        case = dict(cm.FAMILY_CASES[0], mode=mode, Cin2=96)
        assert L.es_conv_kernel_of(C.byref(cm.dummy_conv_args(case, None)), name, 32) == -1 and b'without a fused skip' in L.es_last_error()


def test_a_launch_over_the_descriptor_limit_is_reported_as_chunked(L):
    """rows of the recorded routing table (tests/golden/conv_routes.npz) whose input exceeds 2 GiB supply the arguments"""
    d = np.load(os.path.join(GOLDEN, 'conv_routes.npz'))
    cols, table = [str(c) for c in d['cols']], d['cases']
    ix = {k: cols.index(k) for k in ('O', 'D', 'H', 'W', 'Cin', 'mode')}
    over = []
    for i, row in enumerate(table):
        O, D, H, W, Cin, mode = (int(row[ix[k]]) for k in ('O', 'D', 'H', 'W', 'Cin', 'mode'))
        if mode not in cm.MODE_NAMES:                      # (the table holds invalid arguments too)
            continue
        Di, Hi, Wi = cm.input_dims(mode, (D, H, W))
        if O * Di * Hi * Wi * Cin * 2 >= 1 << 31:
            over.append(i)
    assert len(over) >= 1, 'the recorded table holds no launch over the descriptor limit'
    for i in over[:8]:
        a = _conv_args(cols, table[i])
        name, S = _kernel_of(L, a)
        assert name == 'chunked' and S >= 1, (dict(zip(cols, table[i].tolist())), name, S)
        a.O = 1                                                                         # one object of it: an ordinary launch
        assert _kernel_of(L, a)[0] in cm.KERNELS
