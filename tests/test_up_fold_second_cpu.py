"""CPU-only: what the planner asks for on the two up-sampling convs of the full-width shape step (tools/plan_dryrun.py emits the step
with a CPU Builder; nothing runs).

The folded kernel (ws_256_up_fold: 12 taps per parity class instead of 27) takes unsplit launches only, and a launch that is handed
the shared split-K workspace may be split by the library's tile-quantisation rule.  Builder.conv() therefore asks the library what
the launch does WITHOUT a workspace before it offers one, and withholds it exactly where the answer is the folded kernel:

  * at 32 objects both up-sampling convs carry the folded image, have no workspace and are named ws_256_up_fold, S = 1;
  * with up_fold=False, with deterministic=True and on fp32x the second conv has its workspace and the split the library names for
    those arguments, no folded image, and the shared workspace holds the widest split of the plan;
  * at 16 objects (192 tiles at 16x8x8: not eligible unsplit) the second conv carries the image but keeps workspace and split.
No device compute."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from test_up_fold_cpu import _args, _kernel_of, FOLD, UP_HW      # noqa: E402


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


_packed = {}


def _emit(L, precision='fp16', **kw):
    """the step's Builder; the packed weights of a precision are formed once per module (seconds on the host)"""
    import plan_dryrun
    b, _packed[precision] = plan_dryrun.emit_shape_step_cpu(precision=precision, weights=_packed.get(precision), **kw)
    return b


def _up_ops(b):
    from echoscene_amd import hip
    return [op.u.conv for op in b.ops if op.kind == hip.OP_CONV and op.u.conv.mode == UP_HW]


def _workspace_holds_every_split(L, b):
    from echoscene_amd import hip
    ws = b._ws
    need = 0
    for op in b.ops:
        if op.kind == hip.OP_CONV and op.u.conv.workspace:
            c = op.u.conv
            assert c.workspace == ws.data_ptr(), 'an op points at a workspace that was re-allocated'
            S = L.es_conv_split_of(C.byref(c))
            assert S >= 1
            need = max(need, S * c.O * c.D * c.H * c.W * c.N)
    assert 0 < need <= ws.numel(), (need, ws.numel())


def test_both_up_convs_of_the_plain_plan_are_folded_and_unsplit(L):
    b = _emit(L)
    ups = _up_ops(b)
    assert [(c.O, c.D, c.H, c.W, c.Cin, c.N) for c in ups] == [(32, 16, 8, 8, 672, 672), (32, 16, 16, 16, 448, 448)]
    for c in ups:
        assert c.w2 and not c.a2 and not c.workspace and c.splitk == 0 and c.taps == 27
        assert _kernel_of(L, c) == (FOLD, 1)
        assert L.es_conv_split_of(C.byref(c)) == 1
    _workspace_holds_every_split(L, b)


@pytest.mark.parametrize('kw', [dict(up_fold=False), dict(deterministic=True), dict(precision='fp32x')],
                         ids=['up_fold_off', 'deterministic', 'fp32x'])
def test_the_27_tap_plans_keep_workspace_and_split(L, kw):
    from echoscene_amd.samplers import CANON_OBJECTS
    b = _emit(L, **kw)
    ups = _up_ops(b)
    assert len(ups) == 2
    second = ups[0]
    assert (second.O, second.D, second.H, second.W, second.N) == (32, 16, 8, 8, 672)
    for c in ups:
        assert not c.w2
    assert second.workspace and second.splitk == -1
    # the library's answer for the same arguments, built here from the shape alone
    hint = -CANON_OBJECTS if kw.get('deterministic') else 0
    want = _kernel_of(L, _args(32, (16, 8, 8), second.Cin, 672, w2=0, workspace=True, splitk=-1, o_hint=hint))
    assert _kernel_of(L, second) == want and want[0] != FOLD and want[1] > 1, want
    assert L.es_conv_split_of(C.byref(second)) == want[1]
    if kw == dict(up_fold=False):
        assert want == ('ws_256_8_4_3', 2)                   # tile quantisation: 384 tiles x 2 = 3 full rounds
    _workspace_holds_every_split(L, b)


def test_at_16_objects_the_second_up_conv_keeps_workspace_and_split(L):
    """192 tiles of 256 rows: not the 256-row producer/consumer kernel unsplit, so not the folded one -- the workspace is not withheld"""
    b = _emit(L, O=16)
    second, first = _up_ops(b)
    assert (second.O, second.D, second.H, second.W, second.Cin, second.N) == (16, 16, 8, 8, 672, 672)
    assert second.w2 and second.workspace and second.splitk == -1
    want = _kernel_of(L, _args(16, (16, 8, 8), 672, 672, workspace=True, splitk=-1))
    assert _kernel_of(L, second) == want == _kernel_of(L, _args(16, (16, 8, 8), 672, 672, w2=0, workspace=True, splitk=-1))
    assert want[0] != FOLD and want[1] > 1 and L.es_conv_split_of(C.byref(second)) == want[1]
    assert _kernel_of(L, _args(16, (16, 8, 8), 672, 672))[0] != FOLD            # (unsplit it would not be folded either)
    assert not first.workspace and _kernel_of(L, first) == (FOLD, 1)             # 16^3: 512 tiles, folded as at 32 objects
    _workspace_holds_every_split(L, b)


def test_the_balanced_schedule_is_on_for_the_second_launch_only(L):
    """ConvRoute::fold_bal through es_conv_fold_balanced: three column tiles on a grid that fills under 80 % of its rounds of 256
    workgroups.  The kernel name and the split do not change with it."""
    bal = lambda a: L.es_conv_fold_balanced(C.byref(a))
    second = dict(O=32, dims=(16, 8, 8), Cin=672, N=672)
    assert _kernel_of(L, _args(**second)) == (FOLD, 1) and bal(_args(**second)) == 1              # 384 tiles: 75 % of two rounds
    assert bal(_args(O=32, dims=(16, 16, 16), Cin=448, N=448)) == 0                              # the first launch: two column tiles, 1024 tiles
    full = dict(O=64, dims=(16, 8, 8), Cin=672, N=672)
    assert _kernel_of(L, _args(**full)) == (FOLD, 1) and bal(_args(**full)) == 0                  # 256 row tiles: 768 tiles, three full rounds
    assert bal(_args(O=32, dims=(16, 8, 8), Cin=672, N=896)) == 0                                # four column tiles
    assert bal(_args(w2=0, **second)) == 0                                                       # no folded image: not the folded kernel
    for sk in (-1, 2, 3):                                                                        # any launch with a workspace
        for kw in (second, full, dict(O=32, dims=(16, 16, 16), Cin=448, N=448)):
            assert bal(_args(workspace=True, splitk=sk, **kw)) == 0
    # (too few K units to split: the folded kernel although a workspace is there -- on its plain schedule)
    short = dict(O=32, dims=(16, 8, 8), Cin=32, N=456)
    assert _kernel_of(L, _args(workspace=True, splitk=-1, **short)) == (FOLD, 1)
    assert bal(_args(workspace=True, splitk=-1, **short)) == 0 and bal(_args(**short)) == 1
    # the plan's own ops
    ups = _up_ops(_emit(L))
    assert [bal(c) for c in ups] == [1, 0]
