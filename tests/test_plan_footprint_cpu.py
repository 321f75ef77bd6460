"""CPU-only: what the planners do with memory.  Every plan the volume planner emits (make_vol_plans.CONFIGS) and the layout step
(tools/plan_dryrun.emit_layout_step_cpu at the widths and flags of make_rows_routes.py) goes through tests/plan_footprint.py: every
operand ends inside its buffer; no two ops that a replay leaves unordered (two lanes, or two members of one fused launch) touch the
same bytes with a write among them; every byte of a scratch buffer, and of every other buffer Builder.buf left uninitialised, is
fully written in the same replay before it is read; an op's write overlaps its own read only where ALIASING_OK says so.  The checker
is checked with planted defects in copies of the documents, and the set of configurations the GPU witness runs
(tests/test_hip_plan_footprint.py) is shown to cover every op kind and route.  Nothing runs on a device."""
import copy
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import plan_footprint as pf      # noqa: E402
from plan_footprint import mv    # noqa: E402

ALL = tuple(mv.CONFIGS) + pf.LAYOUT_CONFIGS + tuple(pf.LOOP_CONFIGS)
_cache = {}


def document(name):
    """(extended document, the planner's Builder for the layout step) of a configuration, emitted once per process"""
    if name not in _cache:
        import __graft_entry__ as ge
        ge.build()
        _cache[name] = pf.emit_layout(name)[::-1] if name in pf.LAYOUT_CONFIGS else \
            (pf.emit_layout_loop(name), None) if name in pf.LOOP_CONFIGS else (pf.emit_extended(name), None)
    return _cache[name]


def inputs_of(name, doc):
    return pf.vq_inputs(name, doc) if name in mv.VQ_CONFIGS else pf.step_inputs(doc)


def analyses(name):
    """[Analysis] of the replays of a configuration: the step; for PLMS also iteration 0 (samplers.compose_step_plans: 'first_plan')"""
    key = ('analysis', name)
    if key not in _cache:
        doc, _ = document(name)
        out = [pf.Analysis(name, doc)]
        if doc.get('first_ops') and doc['first_ops'][0]:
            from echoscene_amd.samplers import compose_step_plans
            v = doc['values']
            first = compose_step_plans(doc['ops'], v['n_blend'], v['split'], v['n_eps_ops'], *doc['first_ops'], plms=True)['first_plan']
            out.append(pf.Analysis(name + ' (first iteration)', doc, first))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize('name', ALL)
def test_every_region_ends_inside_its_buffer(name):
    bad = [m for a in analyses(name) for m in a.bounds()]
    assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('name', ALL)
def test_unordered_ops_and_fused_launch_members_touch_disjoint_bytes(name):
    """lane order + FORK / JOIN as es_plan_run enqueues them; the members of one fused launch (plan_dryrun.launches) count as unordered.
    Covers the lane-2 branch, `tiny lanes`, and the shared split-K workspace and statistics scratch: all their users are ordered."""
    bad = [m for a in analyses(name) for m in a.hazards()]
    assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('name', ALL)
def test_scratch_and_uninitialised_bytes_are_written_before_they_are_read(name):
    doc, _ = document(name)
    bad = [m for a in analyses(name) for m in a.defined_before_read(inputs_of(name, doc))]
    assert not bad, '\n'.join(bad[:20])


@pytest.mark.parametrize('name', ALL)
def test_an_op_overlaps_its_own_operands_only_where_listed(name):
    bad = [m for a in analyses(name) for m in a.self_aliasing()]
    assert not bad, '\n'.join(bad[:20])


def test_every_op_kind_has_a_footprint_and_an_aliasing_entry_names_a_kind():
    from echoscene_amd import hip
    kinds = {v for n, v in vars(hip).items() if n.startswith('OP_')}
    assert set(pf.footprint_table()) == kinds == set(mv.kind_members())
    assert set(pf.aliasing_ok()) <= kinds
    for table in pf.aliasing_ok().values():
        assert all(isinstance(reason, str) and len(reason) > 20 for reason in table.values())


def test_plms_state_between_replays_is_not_scratch():
    """first-iteration plan, then the steady plan: the ring and xsave carry state from one replay into the next"""
    from echoscene_amd import hip
    for name in ('tiny plms', 'tiny plms shard 0:3'):
        doc, _ = document(name)
        op = next(op for op in doc['ops'] if op[0] == hip.OP_PLMS)
        f = pf.op_fields(op)
        for field in ('ring', 'xsave', 'x', 'step'):
            size, _, scratch = doc['buffers'][f[field][0]]
            assert not scratch, (name, field)
            assert field in ('x', 'step') or f[field][0] not in doc['empty'], (name, field)       # (x: the caller's input)


@pytest.mark.parametrize('name', pf.LAYOUT_CONFIGS)
def test_layout_regions_lie_inside_the_old_dry_runs_ranges(name):
    """every LINEAR / ROWSEL region the old dry run knows (segments, residuals, outputs) lies inside a range of plan_dryrun._linear_io.
    A step-indexed segment or residual is compared at the row of step 0: the old tool knows nothing of the table's other rows."""
    import plan_dryrun
    from echoscene_amd import hip
    doc, b = document(name)
    n = 0
    for i, (op, rec) in enumerate(zip(b.ops, doc['ops'])):
        if op.kind == hip.OP_LINEAR:
            rd, wr = plan_dryrun._linear_io(op.u.linear, hip)
            old_r, old_w = [(p, p + s) for p, s, _ in rd], [(w[0], w[0] + w[1]) for w in wr]
            stepped = bool(op.u.linear.res_step)
        elif op.kind == hip.OP_ROWSEL:
            a = op.u.rowsel
            old_r, old_w, stepped = [], [(a.out, a.out + 4 * (a.out_ld * (a.rows - 1) + a.n))], False
        else:
            continue
        R, W = pf.op_footprint(doc, rec)
        f = pf.op_fields(rec)
        for g, old in [(g, old_r) for g in R] + [(g, old_w) for g in W]:
            if not (g.field.endswith('.ptr') or g.field in ('res', 'res2', 'out')):
                continue
            # a step-indexed operand (es_seg.step, es_linear_args.res_step; no slabs): the row of step 0 only
            stride = f[g.field[:-3] + 'step_stride'] if g.field.endswith('.ptr') and f[g.field[:-3] + 'step'] else \
                f['res_step_stride'] if g.field == 'res' and stepped else 0
            if stride:
                assert f[g.field[:-3] + 'nslab' if g.field.endswith('.ptr') else 'res_nslab'] <= 1
                if g.off - f[g.field][1] >= 4 * stride:
                    continue
            lo = doc['starts'][g.buf] + g.off
            hi = lo + g.end - g.off
            assert any(a0 <= lo and hi <= a1 for a0, a1 in old), '%s: op %d field %s lies in no range of the old dry run' % (name, i, g.field)
            n += 1
    assert n > 100


# ------------------------------------------------------------------------------------------------ the checker checked
def _tiny():
    doc, _ = document('tiny')
    return copy.deepcopy(doc)


def _findings(doc, ops=None):
    a = pf.Analysis('planted', doc, ops)
    return a, a.all_findings(pf.step_inputs(doc))


def _idx(doc, name):
    return mv.field_names()[mv.kind_members()[doc[0]]].index(name) + 2


def test_planted_join_behind_the_first_reader_of_a_lane_result():
    from echoscene_amd import hip
    doc = _tiny()
    a = pf.Analysis('tiny', doc)
    j = next(i for i, op in enumerate(doc['ops']) if op[0] == hip.OP_JOIN)
    side_w = [g for i, (R, W) in enumerate(a.fp) if doc['ops'][i][1] == 2 for g in W]
    k, field = next((i, g.field) for i in range(j + 1, len(a.fp)) for g in a.fp[i][0] if any(pf.regions_overlap(g, w) for w in side_w))
    ops = doc['ops'][:j] + doc['ops'][j + 1:k + 1] + [doc['ops'][j]] + doc['ops'][k + 1:]
    _, bad = _findings(doc, ops)
    assert any('op %d (%s) field %s reads' % (k - 1, pf.kind_name(ops[k - 1][0]), field) in m and 'unordered' in m for m in bad), bad[:5]


def _widest(doc, kind, field):
    """(op index, its region, buffer) of the op whose declared extent in ``field`` ends last"""
    a = pf.Analysis('tiny', doc)
    best = None
    for i, (R, W) in enumerate(a.fp):
        for g in W:
            if doc['ops'][i][0] == kind and g.field == field and (best is None or g.end > best[1].end):
                best = (i, g)
    return best


def test_planted_workspace_one_slab_short():
    from echoscene_amd import hip
    doc = _tiny()
    i, g = _widest(doc, hip.OP_CONV, 'workspace')
    f = pf.op_fields(doc['ops'][i])
    slab = f['O'] * f['D'] * f['H'] * f['W'] * f['N'] * 4
    assert doc['buffers'][g.buf][0] == g.end and g.end % slab == 0 and g.end // slab > 1       # the workspace holds exactly its widest user
    doc['buffers'][g.buf][0] -= slab
    _, bad = _findings(doc)
    assert any('op %d (CONV) field workspace: ends %d bytes past' % (i, slab) in m for m in bad), bad[:5]


def test_planted_statistics_scratch_one_float_short():
    """(the shipped scratch is sized for the smallest voxel tile and is larger than any route needs: `short` is measured from the
    widest user, as for the workspace)"""
    from echoscene_amd import hip
    doc = _tiny()
    i, g = _widest(doc, hip.OP_GN, 'stats')
    assert doc['buffers'][g.buf][0] >= g.end
    doc['buffers'][g.buf][0] = g.end - 4
    _, bad = _findings(doc)
    assert any('op %d (GN) field stats: ends 4 bytes past' % i in m for m in bad), bad[:5]


def test_planted_loop_state_flagged_scratch():
    doc = _tiny()
    x = doc['tensors']['x'][1][0]
    doc['buffers'][x][2] = True
    a, bad = _findings(doc)
    first = min(i for i, (R, W) in enumerate(a.fp) for g in R if g.buf == x)
    assert any('op %d (%s) field x: reads' % (first, pf.kind_name(doc['ops'][first][0])) in m and 'scratch buffer %d' % x in m for m in bad), bad[:5]


def test_planted_swap_of_two_dependent_ops():
    from echoscene_amd import hip
    doc = _tiny()
    i = next(i for i, op in enumerate(doc['ops']) if op[0] == hip.OP_GN and doc['ops'][i + 1][0] == hip.OP_CONV)
    y = pf.op_fields(doc['ops'][i])['y_f16']
    assert pf.op_fields(doc['ops'][i + 1])['a'] == y
    ops = list(doc['ops'])
    ops[i], ops[i + 1] = ops[i + 1], ops[i]
    _, bad = _findings(doc, ops)
    assert any('op %d (CONV) field a: reads' % i in m and 'buffer %d ' % y[0] in m for m in bad), bad[:5]


def test_planted_lane_product_writing_into_a_concurrent_convs_output():
    from echoscene_amd import hip
    doc = _tiny()
    j = next(i for i, op in enumerate(doc['ops']) if op[0] == hip.OP_JOIN)
    conv = next(i for i, op in enumerate(doc['ops'][:j]) if op[0] == hip.OP_CONV and op[1] == 0)
    lin = max(i for i, op in enumerate(doc['ops'][:j]) if op[0] == hip.OP_LINEAR and op[1] == 2)
    doc['ops'][lin][_idx(doc['ops'][lin], 'out')] = list(pf.op_fields(doc['ops'][conv])['out_f32'])
    _, bad = _findings(doc)
    assert any(('op %d (LINEAR) field out' % lin) in m and ('op %d (CONV)' % conv) in m and 'unordered' in m for m in bad), bad[:5]


def test_planted_fused_member_reading_its_neighbours_output():
    from echoscene_amd import hip
    doc = _tiny()
    i = next(i for i, op in enumerate(doc['ops']) if op[0] == hip.OP_LINEAR and pf.op_fields(op)['fuse_next'])
    assert doc['ops'][i + 1][0] == hip.OP_LINEAR and pf.launch_groups(doc['ops'])[[g[0] for g in pf.launch_groups(doc['ops'])].index(i)][1] >= 2
    doc['ops'][i + 1][_idx(doc['ops'][i + 1], 'seg[0].ptr')] = list(pf.op_fields(doc['ops'][i])['out'])
    _, bad = _findings(doc)
    assert any('op %d (LINEAR) field seg[0].ptr reads what op %d (LINEAR) field out writes: members of one fused launch' % (i + 1, i) in m
               for m in bad), bad[:5]


# ------------------------------------------------------------------------------------------------ what the GPU witness covers
def _routes(name):
    """{(kind, route detail)} of a configuration: GN by statistics source, CONV by split / unsplit and by the sums it leaves"""
    from echoscene_amd import hip
    doc, _ = document(name)
    out = set()
    for op in doc['ops'] + [o for o in doc.get('first_ops', []) if o]:
        if op[0] in (hip.OP_FORK, hip.OP_JOIN):
            continue
        out.add((op[0], ''))
        if op[0] == hip.OP_GN:
            out.add((op[0], 'stats_src=' + hip.GN_STATS_SOURCES[pf.gn_route(op[0], op[2:]).stats_src]))
        if op[0] == hip.OP_CONV:
            r, f = pf.conv_route(op[0], op[2:]), pf.op_fields(op)
            out.add((op[0], 'split' if r.reduce else 'unsplit'))
            if f['gn_stats_out']:
                out.add((op[0], 'gn_stats_out'))
            if f['gn_part_out'] and r.reduce == 2:
                out.add((op[0], 'gn_part_out'))
    return out


def test_the_witnessed_configurations_cover_every_kind_and_route():
    need = set().union(*[_routes(n) for n in ALL])
    have = set().union(*[_routes(n) for n in pf.WITNESSED])
    assert not need - have, sorted((pf.kind_name(k), d) for k, d in need - have)


def test_never_poisoned_tensors_are_a_negligible_share():
    """int32 / int64 tensors (graph indices, the step counter) are never poisoned by the witness: under 0.01 % of the bytes of every
    recorded volume plan and of the witnessed layout steps"""
    docs, _ = mv.load()
    for name in list(docs) + [n for n in pf.WITNESSED if n not in docs]:
        d = docs[name] if name in docs else document(name)[0]
        ints = sum(b[0] for b in d['buffers'] if set(b[1]) & {'int32', 'int64'})
        share = ints / sum(b[0] for b in d['buffers'])
        print('%-28s never poisoned: %d bytes, %.6f %%' % (name, ints, 100 * share))
        assert share < 1e-4, (name, share)
    assert set(pf.WITNESSED) <= set(ALL)


def test_emitted_documents_are_the_recorded_ones():
    """the extension adds keys and changes nothing: the analysed op streams are those of tests/golden/vol_plans.npz"""
    import json
    docs, _ = mv.load()
    for name in mv.CONFIGS:
        got = json.loads(json.dumps(document(name)[0]['ops']))
        assert got == docs[name]['ops'], name
