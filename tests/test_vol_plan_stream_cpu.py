"""CPU-only: the op stream of every plan the volume planner emits (tests/golden/make_vol_plans.py: the shape step of the tiny network
in every variant a caller can ask for, the full-width step at 32 and 16 objects, the VQ-VAE decoder and encoder) against the recorded
file tests/golden/vol_plans.npz, field by field.  The planner only decides WHAT the library is asked to do; this is the check that a
change of the planner's code leaves that untouched.  Nothing runs on a device."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import make_vol_plans as mv      # noqa: E402


@pytest.fixture(scope='module')
def recorded():
    import __graft_entry__ as ge
    ge.build()
    docs, fields = mv.load()
    assert fields == mv.field_names(), 'the argument structs changed: the recorded streams do not describe them'
    return docs


def op_diff(got, want, what):
    """the first field in which two canonical ops differ, named; None when they are equal"""
    if got is None or want is None:
        return None if got is want else '%s: %s, recorded %s' % (what, 'absent' if got is None else 'present', 'absent' if want is None else 'present')
    if got[0] != want[0]:
        return '%s: kind %d, recorded %d' % (what, got[0], want[0])
    if got[1] != want[1]:
        return '%s: lane %d, recorded %d' % (what, got[1], want[1])
    member = mv.kind_members()[got[0]]
    names = mv.field_names()[member] if member else []
    assert len(got) == len(want) == 2 + len(names)
    for n, g, w in zip(names, got[2:], want[2:]):
        if g != w:
            return '%s (kind %d): field %s = %r, recorded %r' % (what, got[0], n, g, w)
    return None


def doc_diff(got, want):
    """every difference between an emitted and a recorded document by name (the first differing field of each op)"""
    bad = []
    if len(got['ops']) != len(want['ops']):
        bad.append('%d ops, recorded %d' % (len(got['ops']), len(want['ops'])))
    for i, (g, w) in enumerate(zip(got['ops'], want['ops'])):
        bad.append(op_diff(g, w, 'op %d' % i))
    for i in range(2):
        bad.append(op_diff(got['first_ops'][i], want['first_ops'][i], 'first_ops[%d]' % i))
    for key in ('weight_bytes', 'flops', 'tags', 'values', 'tensors'):
        g, w = got.get(key), want.get(key)
        if isinstance(w, dict) and isinstance(g, dict):
            bad += ['%s[%r] = %r, recorded %r' % (key, k, g.get(k), w.get(k)) for k in sorted(set(g) | set(w)) if g.get(k) != w.get(k)]
        elif g != w:
            bad.append('%s = %r, recorded %r' % (key, g, w))
    if len(got['buffers']) != len(want['buffers']):
        bad.append('%d buffers, recorded %d' % (len(got['buffers']), len(want['buffers'])))
    bad += ['buffer %d = (bytes, dtypes, scratch) %r, recorded %r' % (i, g, w)
            for i, (g, w) in enumerate(zip(got['buffers'], want['buffers'])) if g != w]
    return [m for m in bad if m]


def test_the_file_holds_every_configuration(recorded):
    assert sorted(recorded) == sorted(mv.CONFIGS)


@pytest.mark.parametrize('name', mv.CONFIGS)
def test_plan_stream_equals_the_recorded_one(recorded, name):
    import json
    got = json.loads(json.dumps(mv.document(name)))          # (tuples -> lists, as in the file)
    bad = doc_diff(got, recorded[name])
    assert not bad, 'configuration %r: %d differences\n  ' % (name, len(bad)) + '\n  '.join(bad[:20])


def _planner_source():
    with open(os.path.join(ROOT, 'echoscene_amd', 'plan_vol.py')) as f:
        return f.read()


def test_the_file_covers_every_op_kind_the_volume_emitters_push(recorded):
    """every hip.OP_* the planner's source names is the kind of some recorded op"""
    from echoscene_amd import hip
    named = sorted(set(re.findall(r'\bhip\.(OP_\w+)', _planner_source())))
    assert len(named) >= 15, named
    seen = {op[0] for d in recorded.values() for op in d['ops'] + [o for o in d['first_ops'] if o]}
    # (the PLMS first-iteration kinds are named by the sampler layer, which hands them to Builder.plms)
    for n in named + ['OP_PLMS', 'OP_PLMS_FIRST_A', 'OP_PLMS_FIRST_B', 'OP_DDIM_BLEND', 'OP_DDIM_BLEND_VOX']:
        assert getattr(hip, n) in seen, 'no recorded plan holds an op of kind %s' % n


@pytest.mark.parametrize('member,kinds,at_least', [('conv', ('OP_CONV', 'OP_CONV_F32'), 25), ('gn', ('OP_GN',), 18)])
def test_every_field_the_planner_assigns_is_set_in_some_recorded_op(recorded, member, kinds, at_least):
    """a ConvArgs (GNArgs) field that plan_vol.py assigns is non-zero in at least one recorded op: no emitter path goes unrecorded"""
    from echoscene_amd import hip
    names = mv.field_names()[member]
    assigned = set()
    for line in _planner_source().splitlines():
        m = re.match(r'^([^=#]*[^=!<>#\s])\s*=(?!=)', line)
        if m:
            assigned |= {f for f in names if re.search(r'\.%s\b' % f, m.group(1))}
    assert len(assigned) >= at_least, sorted(assigned)
    kinds = [getattr(hip, k) for k in kinds]
    for f in sorted(assigned):
        k = 2 + names.index(f)
        assert any(op[k] for d in recorded.values() for op in d['ops'] if op[0] in kinds), \
            '%s.%s is zero in every recorded op' % (member, f)
