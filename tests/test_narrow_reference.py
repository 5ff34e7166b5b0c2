"""The independent numpy narrow phase of support_narrow.py, held to the oracle and to closed forms (CPU).

Every directed case and every seeded scene that tests/test_gpu_narrow_ground.py runs on the device goes through ref_ground_contacts and
through oracle.forward_debug here: count, order and ids equal, position, normal and distance to 1e-12 (the bound test_oracle_contacts.py
uses for analytic geometry).  A handful of closed forms pin the reference by more than agreement, every case of the table must be
admissible (a discrete decision may then differ on the device only through a bug), and the seeded draw may reject at most 10 %."""
import numpy as np
import pytest

import support_narrow as sn
from support_narrow import (ref_ground_contacts, admissible, contact_frame, directed_cases, directed_model, directed_batches, seeded_scenes,
                            build_model, rot, quat_to_mat, mat_to_quat, plane_from_normal, SPHERE, BOX, CYLINDER, I4, ORIGIN)

TOL = 1e-12


def _arrays(r):
    c = r['contacts']
    return (np.array([x[2] for x in c]).reshape(-1, 3), np.array([x[3] for x in c]).reshape(-1, 3), np.array([x[4] for x in c]),
            np.array([x[0] for x in c], int), np.array([x[1] for x in c], int))


def _check_vs_oracle(oracle, m, qpos, label):
    r = ref_ground_contacts(m, qpos)
    fd = oracle.forward_debug(m, qpos, np.zeros(m.nv))
    n = len(r['contacts'])
    assert fd['ncon'] == n, (label, fd['ncon'], n)
    pos, nrm, dist, g1, g2 = _arrays(r)
    oc = fd['contact'][:n]
    assert np.array_equal(oc[:, 15].astype(int), g1) and np.array_equal(oc[:, 16].astype(int), g2), (label, oc[:, 15:17], g1, g2)
    err = 0.0
    if n:
        frames = np.array([contact_frame(x) for x in nrm])
        err = max(np.abs(pos - oc[:, :3]).max(), np.abs(frames - oc[:, 3:12]).max(), np.abs(dist - oc[:, 17]).max())
    assert err < TOL, (label, err)
    return r, err


@pytest.mark.parametrize('key', list(directed_batches()))
def test_directed_cases_are_admissible_and_match_the_oracle(oracle, key):
    m = directed_model(key)
    for c in directed_batches()[key]:
        ok, why = admissible(m, c.qpos, exact=c.exact)
        assert ok, (c.name, why)
        ok, why = admissible(m, c.qpos.astype(np.float32).astype(float), exact=c.exact)      # the pose the device holds
        assert ok, (c.name, 'rounded to fp32', why)
        assert np.abs(c.qpos[:3]).max() < 0.5
        r, _ = _check_vs_oracle(oracle, m, c.qpos, c.name)
        assert len(r['contacts']) == c.ncon, (c.name, len(r['contacts']), c.ncon)
        assert r['full'] == c.truncated, c.name
        status = int(oracle.step(m, c.qpos[None], np.zeros((1, m.nv)))['status'][0])
        assert status == (sn.FMJ_WARN_CONTACTFULL if c.truncated else 0), (c.name, status)
    assert len(directed_batches()[key]) % 2 == 1                      # odd batches: the two halves of a wave never pair up evenly
    counts = [c.ncon for c in directed_batches()[key]]                  # neighbouring envs disagree about the count (the exact grid cases all
    assert all(a != b for a, b in zip(counts, counts[1:])) or key == 'grid_sphere', (key, counts)      # give one contact: they differ in the cell)


def _case(name):
    c = [c for c in directed_cases() if c.name == name]
    assert len(c) == 1, name
    return directed_model(c[0].model), c[0], ref_ground_contacts(directed_model(c[0].model), c[0].qpos)


def test_the_table_reaches_the_branches_it_names():
    """What each directed case is in the table for, read back from the reference's own decisions."""
    seeds = {k: [d[1] for d in _case(k + '_in2mm')[2]['decisions'] if d[0] == 'seed'] for k in ('sphere_ny045', 'sphere_ny055', 'sphere_ny-08', 'sphere_tilt_y')}
    assert seeds == {'sphere_ny045': [False], 'sphere_ny055': [True], 'sphere_ny-08': [True], 'sphere_tilt_y': [False]}
    assert _case('sphere_ny-08_in2mm')[2]['contacts'][0][3][1] < -0.5 and abs(_case('sphere_tilt_y_in2mm')[2]['contacts'][0][3][1]) < 1e-15
    # capsule: which end
    pen = lambda name: [d[2] for d in _case(name)[2]['decisions'] if d[0] != 'seed' and d[3]]
    assert pen('capsule_plus_end_only') == [0] and pen('capsule_minus_end_only') == [1] and pen('capsule_both_ends') == [0, 1]
    d = [c[4] for c in _case('capsule_parallel')[2]['contacts']]
    assert abs(d[0] - d[1]) < 1e-12
    # box: corners kept = the first four penetrating in corner order
    assert pen('box_flat') == [0, 1, 2, 3] and pen('box_flipped') == [4, 5, 6, 7] and len(pen('box_on_edge')) == 2 and len(pen('box_on_corner')) == 1
    for name, nbelow in (('box_5_below', 5), ('box_8_below', 8)):
        m, c, r = _case(name)
        below = pen(name)
        assert len(below) == nbelow and len(r['contacts']) == 4
        co = np.array(sn._corners((0.03, 0.02, 0.012)))
        R, t = quat_to_mat(c.qpos[3:7]/np.linalg.norm(c.qpos[3:7])), c.qpos[:3]
        for k, con in zip(below[:4], r['contacts']):
            assert np.allclose(con[2] + con[3]*con[4]/2, t + R @ co[k], atol=1e-15)      # the record sits half the depth above corner k
    # cylinder: fallback direction, flip of the near disk
    cy = lambda name: [d[3:] for d in _case(name)[2]['decisions'] if len(d) > 2 and d[2] == 'cyl'][0]      # (flip, fallback)
    assert cy('cylinder_upright_exact') == (True, True) and cy('cylinder_upside_down_exact') == (False, True)
    assert cy('cylinder_tilt30_two') == (True, False) and cy('cylinder_tilt150_two') == (False, False) and cy('cylinder_on_side')[1] is False
    # heightfield: cells and triangles of the exact cases (column, row, upper triangle)
    where = lambda name: [d[4] for d in _case(name)[2]['decisions'] if d[0] != 'seed'][0]
    assert where('grid_column_line') == (3, 4, True) and where('grid_row_line') == (2, 6, False) and where('grid_diagonal') == (5, 1, False)
    assert where('grid_node') == (4, 2, False) and where('grid_first_node') == (0, 0, False)
    assert where('grid_last_column') == (7, 3, False) and where('grid_last_row') == (1, 7, True) and where('grid_far_corner') == (7, 7, False)
    assert where('grid_outside') == (None, None, None)
    for c in directed_cases():
        if c.exact:      # dyadic coordinates: the grid coordinates are exact numbers, and the same ones in float32
            g64 = ref_ground_contacts(directed_model(c.model), c.qpos)['candidates'][0]['grid']
            g32 = ref_ground_contacts(directed_model(c.model), c.qpos.astype(np.float32), dtype=np.float32)['candidates'][0]['grid']
            assert g64 == g32 and all(float(x*64).is_integer() for x in g64), (c.name, g64, g32)
    for pre in ('hf', 'hfr'):
        lo, up = where(pre + '_sphere_lower_triangle'), where(pre + '_sphere_upper_triangle')
        assert lo[:2] == up[:2] and (lo[2], up[2]) == (False, True)              # the two triangles of ONE cell
        n = [c[3] for c in _case(pre + '_capsule_two_triangles')[2]['contacts']]
        assert len(n) == 2 and np.degrees(np.arccos(n[0] @ n[1])) > 5            # the two ends meet different slopes
        r = _case(pre + '_box_over_the_edge')[2]
        assert sum(1 for c in r['candidates'] if not np.isfinite(c['dist'])) >= 2 and len(r['contacts']) == 2
        slopes = [np.degrees(np.arccos(quat_to_mat(np.asarray(sn.MODELS[pre + '_sphere'][0][0][4], float))[:, 2] @ c[3]))
                  for name in ('_sphere_lower_triangle', '_cylinder_on_slope', '_capsule_two_triangles') for c in _case(pre + name)[2]['contacts']]
        assert max(slopes) > 10
    # the rotated heightfield sees the same ground-frame configuration
    for name in ('_sphere_lower_triangle', '_capsule_two_triangles', '_box_over_the_edge', '_cylinder_on_slope', '_cylinder_on_side_slope'):
        a, b = _case('hf' + name)[2], _case('hfr' + name)[2]
        assert np.allclose([c[4] for c in a['contacts']], [c[4] for c in b['contacts']], atol=1e-12)
    # two grounds: contacts on both, ground-major; chunking: 20 to 48 contacts on both sides of geom 64
    for name in ('two_grounds_a', 'two_grounds_shallow'):
        g1 = [c[0] for c in _case(name)[2]['contacts']]
        assert g1 == sorted(g1) and g1.count(0) >= 2 and g1.count(1) >= 2
    assert min(c[4] for c in _case('two_grounds_shallow')[2]['contacts']) > -0.01
    for name in ('chunk_low_x', 'chunk_shallow'):
        m, c, r = _case(name)
        g2 = np.array([x[1] for x in r['contacts']])
        assert m.ngeom == 77 and m.max_contacts == 48 and 20 <= len(g2) <= 48 and not r['full'], (name, len(g2))
        assert (g2 >= 64).sum() >= 4 and (g2 < 64).sum() >= 4 and np.array_equal(g2, np.sort(g2)), (name, g2)
    assert min(c[4] for c in _case('chunk_shallow')[2]['contacts']) > -0.01
    m, c, r = _case('truncate_two_flat_boxes')
    assert r['total'] == 8 and [x[1] for x in r['contacts']] == [1, 1, 1, 1, 2, 2] and m.max_contacts == 6


# ---- closed forms on the reference itself -------------------------------------------------------------------------------------------
def test_sphere_on_a_tilted_plane_closed_form():
    n = np.array([0.3, -0.4, np.sqrt(0.75)])
    pl = plane_from_normal(n, pos=(0.01, 0.02, 0.03))
    m = build_model([pl], [(SPHERE, (0.02,), (0.01, 0.0, -0.01), I4)], max_contacts=4)
    R = rot((1, 2, 3), 0.7)
    t = np.array([0.05, -0.04, 0.03])
    t -= n*(n @ (t + R @ np.array([0.01, 0.0, -0.01]) - np.array(pl[1])) - 0.016)      # the sphere's centre 16 mm above the plane: 4 mm in
    q = np.concatenate([t, mat_to_quat(R)])
    c = t + R @ np.array([0.01, 0.0, -0.01])
    d = n @ (c - np.array(pl[1])) - 0.02
    assert abs(d + 0.004) < 1e-15
    r = ref_ground_contacts(m, q)
    assert len(r['contacts']) == 1
    g1, g2, pos, nrm, dist = r['contacts'][0]
    assert (g1, g2) == (0, 1) and abs(dist - d) < 1e-15 and np.allclose(nrm, n, atol=1e-15)
    assert np.allclose(pos, c - n*(0.02 + d/2), atol=1e-15)                   # pos = c - n (r + d / 2)
    f = contact_frame(nrm).reshape(3, 3)
    assert np.allclose(f @ f.T, np.eye(3), atol=1e-15) and np.allclose(np.cross(f[0], f[1]), f[2], atol=1e-15)
    assert abs(f[1] @ [0, 1, 0]) > abs(f[1] @ [0, 0, 1])                       # |n_y| <= 0.5: t1 comes from (0, 1, 0)
    f = contact_frame(np.array([0.0, 0.6, 0.8]))
    assert np.allclose(f[3:6], [0, -0.8, 0.6], atol=1e-15)                     # |n_y| > 0.5: (0, 0, 1) made orthogonal


def test_flat_box_closed_form():
    sx, sy, sz = 0.03, 0.02, 0.012
    m = build_model([('plane', ORIGIN, I4)], [(BOX, (sx, sy, sz), ORIGIN, I4)], max_contacts=8)
    r = ref_ground_contacts(m, np.array([0.1, -0.05, sz - 0.002, 1.0, 0, 0, 0]))
    assert len(r['contacts']) == 4
    for k, (g1, g2, pos, nrm, dist) in enumerate(r['contacts']):              # the four corners at (+-sx, +-sy), x fastest, 1 mm below the plane
        assert np.allclose(pos, [0.1 + (sx if k & 1 else -sx), -0.05 + (sy if k & 2 else -sy), -0.001], atol=1e-15)
        assert abs(dist + 0.002) < 1e-15 and np.array_equal(nrm, [0, 0, 1])


def test_upright_cylinder_closed_form():
    rad, h = 0.02, 0.004
    m = build_model([('plane', ORIGIN, I4)], [(CYLINDER, (rad, h), ORIGIN, I4)], max_contacts=8)
    r = ref_ground_contacts(m, np.array([0.0, 0.0, h - 0.002, 1.0, 0, 0, 0]))
    assert len(r['contacts']) == 3                                            # three rim points 120 degrees apart, the first on the geom's +x
    P = np.array([c[2] for c in r['contacts']])
    assert np.allclose(P[:, 2], -0.001, atol=1e-15) and np.allclose(np.hypot(P[:, 0], P[:, 1]), rad, atol=1e-15)
    assert np.allclose(P[0, :2], [rad, 0], atol=1e-15)
    ang = np.sort(np.mod(np.arctan2(P[:, 1], P[:, 0]), 2*np.pi))
    assert np.allclose(np.diff(ang), 2*np.pi/3, atol=1e-12)
    # tilted by 30 degrees about y: the deepest rim point is where the near rim dips lowest, the second is the same point of the far disk
    R = rot((0, 1, 0), np.pi/6)
    t = np.array([0.0, 0.0, -0.005])
    r = ref_ground_contacts(m, np.concatenate([t, mat_to_quat(R)]))
    assert len(r['contacts']) == 4
    P = np.array([c[2] + c[3]*c[4]/2 for c in r['contacts']]) - t             # the points on the cylinder
    assert np.allclose(P[0], R @ np.array([rad, 0.0, -h]), atol=1e-15) and np.allclose(P[1], R @ np.array([rad, 0.0, h]), atol=1e-15)
    side = sorted(map(tuple, np.round(P[2:] @ R, 12)))                          # back in the geom frame
    assert np.allclose(side, [(-rad/2, -rad*np.sqrt(0.75), -h), (-rad/2, rad*np.sqrt(0.75), -h)], atol=1e-11)
    assert np.allclose([c[4] for c in r['contacts']], P[:, 2] + t[2], atol=1e-15)


def test_linear_ramp_heightfield_closed_form():
    """z = a x + b y sampled on a grid: both triangles of every cell lie in the ramp, n = (-a, -b, 1) / |.| and dist = n . (p - p_ramp)."""
    a, b, zs = 0.3, -0.2, 0.05
    nr, nc, rx, ry = 5, 7, 0.3, 0.2
    xs, ys = np.linspace(-rx, rx, nc), np.linspace(-ry, ry, nr)
    data = (a*xs[None, :] + b*ys[:, None])/zs
    m = build_model([('hfield', data, (rx, ry, zs, 0.1), ORIGIN, I4)], [(SPHERE, (0.02,), ORIGIN, I4)], max_contacts=4)
    n = np.array([-a, -b, 1.0])/np.sqrt(a*a + b*b + 1)
    seen = set()
    for x, y in ((0.03, 0.01), (0.01, 0.03), (-0.22, 0.13), (-0.21, 0.17), (0.28, -0.19)):
        c = np.array([x, y, a*x + b*y + 0.015])
        r = ref_ground_contacts(m, np.concatenate([c, [1.0, 0, 0, 0]]))
        (g1, g2, pos, nrm, dist), = r['contacts']
        assert np.allclose(nrm, n, atol=1e-14) and abs(dist - (n[2]*0.015 - 0.02)) < 1e-15
        assert np.allclose(pos, c - n*(0.02 + dist/2), atol=1e-15)
        seen.add(r['decisions'][0][4][2])
    assert seen == {False, True}                                                # points in lower and in upper triangles


def test_seeded_scenes_match_the_oracle_and_few_draws_are_rejected(oracle):
    sc = seeded_scenes()
    share = sc.rejected/sc.draws
    print(f'seeded scenes: {sc.draws} draws, {sc.rejected} rejected ({100*share:.1f} %)')
    assert share <= 0.10, (sc.draws, sc.rejected)
    assert len(sc.two_grounds) == 8 and len(sc.single) == 8 and len(sc.mesh) == 4 and all(len(s[2]) == 3 for s in sc.two_grounds + sc.single + sc.mesh)
    total, worst, both, meshc = 0, 0.0, 0, 0
    for group in (sc.two_grounds, sc.single, sc.mesh):
        for i, (grounds, geoms, qs) in enumerate(group):
            m = build_model(grounds, geoms, max_contacts=32)
            for q in qs:
                assert admissible(m, q)[0] and admissible(m, q.astype(np.float32).astype(float))[0]
                r, err = _check_vs_oracle(oracle, m, q, (i, q))
                total += len(r['contacts']); worst = max(worst, err)
                g1 = {c[0] for c in r['contacts']}
                both += len(g1) == 2
                meshc += sum(1 for c in r['contacts'] if m.geom_type[c[1]] == sn.MESH)
    print(f'seeded scenes: {total} contacts, worst difference to the oracle {worst:.1e}, {both} poses touch both grounds, {meshc} mesh contacts')
    assert total >= 150 and both >= 6 and meshc >= 12
