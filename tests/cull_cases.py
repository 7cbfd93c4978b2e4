"""Hand-built KeyFrameCulling cases for tests/test_cull_cases_cpu.py and tests/test_cull_gpu.py, each with its twin on the other
side of the gate it probes.  A case is dict(q, cand, flags, mono, th, want): the problem of tests/cull_ref.py, the candidates and
their flags, and the hand answer -- the fields of the result that the case is about, worked out below from the reference's text.

Keyframe 0 is the candidate A (1 is B where a case has two); keyframes 2 .. are the bystanders X, Y, Z, W.  An entry is (kf,
octave, stereo, depth).  `red(A)` is a point A sees redundantly: A and three others, all mono at octave 0, so Observations() = 4 >
3 and three others pass the octave test.  `lone(A)` is a point with A and two others: Observations() = 3, never redundant."""
import numpy as np

import cull_ref as R

A, B, X, Y, Z, W = 0, 1, 2, 3, 4, 5
TH = 40.0
ABOVE_TH = float(np.nextafter(np.float32(TH), np.float32(np.inf)))


def ent(kf, octave=0, stereo=0, depth=1.0):
    return (kf, octave, stereo, depth)


def red(kf, octave=0, depth=1.0):
    return [ent(kf, octave, 0, depth), ent(X), ent(Y), ent(Z)]


def lone(kf):
    return [ent(kf), ent(X), ent(Y)]


def case(points, cand=(A,), flags=None, mono=0, th=TH, n_kf=6, want=None, **kw):
    flags = [0] * len(cand) if flags is None else flags
    return dict(q=R.problem(points, n_kf, **kw), cand=np.array(cand, np.int32), flags=np.array(flags, np.uint8), mono=mono, th=th,
                want=want or {})


def ratio(n_red, n):
    """n points in A, n_red of them redundant: culled iff (double)n_red > 0.9 * (double)n"""
    culled = n_red * 10 > n * 9                                             # the same comparison in integers
    assert (float(n_red) > 0.9 * float(n)) == culled                        # 0.9 * 10, 20, 30 are exact in double
    return case([red(A)] * n_red + [lone(A)] * (n - n_red), want=dict(verdict=[R.CULLED if culled else R.KEPT], counts2=[[n_red, n]]))


def sized(P):
    """P points in A: all redundant but the last, which has Observations() = 3 and goes bad (2 <= 2) when A is culled; its
    other two entries are cleared.  Crosses the lane-ownership boundary of a 1024-lane workgroup at 1023 / 1024 / 1025."""
    pts = [red(A)] * (P - 1) + [lone(A) if P > 1 else red(A)]
    n_red = P - 1 if P > 1 else 1
    dead = np.zeros(sum(len(o) for o in pts), np.uint8)
    dead[np.arange(P - 1) * 4] = 1
    bad = np.zeros(P, np.uint8)
    if P > 1:
        dead[(P - 1) * 4:] = (1, 2, 2)
        bad[P - 1] = 1
    else:
        dead[0] = 1
    return case(pts, want=dict(verdict=[R.CULLED], counts2=[[n_red, P]], obs_dead=dead, point_bad=bad,
                               info8=[0, 1, 0, int((dead != 0).sum()), int(bad.sum()), 0, 0, 0]))


def cascade(order):
    """A sees 30 redundant points and 2 points (A, B, X); B sees 10 redundant points and those 2.  Alone, B is 10 of 12 = 0.83:
    kept.  A is 30 of 32 = 0.94: culled, which takes the two shared points to nObs 2: they go bad, B is 10 of 10: culled.
    order (A, B) culls both; order (B, A) keeps B."""
    pts = [red(A)] * 30 + [[ent(A), ent(B), ent(X)]] * 2 + [red(B)] * 10
    if order == (A, B):
        want = dict(verdict=[R.CULLED, R.CULLED], counts2=[[30, 32], [10, 10]])
        bad = [0] * 30 + [1, 1] + [0] * 10
    else:
        want = dict(verdict=[R.KEPT, R.CULLED], counts2=[[10, 12], [30, 32]])
        bad = [0] * 30 + [1, 1] + [0] * 10
    want["point_bad"] = bad
    return case(pts, cand=order, want=want)


def cases():
    c = {}
    # nRedundant against 0.9 * nMPs
    for n_red, n in ((9, 10), (10, 10), (19, 20), (18, 20), (27, 30), (28, 30)):
        c[f"ratio_{n_red}_of_{n}"] = ratio(n_red, n)
    c["no_points"] = case([red(B)], want=dict(verdict=[R.KEPT], counts2=[[0, 0]]))          # 0 > 0.0 is false
    # Observations() of exactly 3 and of 4
    c["observations_3"] = case([lone(A)], want=dict(verdict=[R.KEPT], counts2=[[0, 1]]))
    c["observations_4"] = case([red(A)], want=dict(verdict=[R.CULLED], counts2=[[1, 1]]))
    # two stereo observations: nObs is 4 but there is ONE other keyframe; with three others it is redundant
    c["two_stereo"] = case([[ent(A, stereo=1), ent(X, stereo=1)]], want=dict(verdict=[R.KEPT], counts2=[[0, 1]], n_obs=[4]))
    c["two_stereo_twin"] = case([[ent(A, stereo=1), ent(X, stereo=1), ent(Y), ent(Z)]], want=dict(verdict=[R.CULLED], counts2=[[1, 1]]))
    # octave_i == octave + 1 counts, octave + 2 does not
    c["octave_plus_1"] = case([[ent(A, 0), ent(X, 1), ent(Y, 1), ent(Z, 1)]], want=dict(verdict=[R.CULLED], counts2=[[1, 1]]))
    c["octave_plus_2"] = case([[ent(A, 0), ent(X, 1), ent(Y, 2), ent(Z, 1)]], want=dict(verdict=[R.KEPT], counts2=[[0, 1]]))
    # the candidate's own entry as one of only three: Observations() = 4 through A's stereo weight, two others
    c["own_entry_of_three"] = case([[ent(X), ent(A, stereo=1), ent(Y)]], want=dict(verdict=[R.KEPT], counts2=[[0, 1]]))
    c["own_entry_of_four"] = case([[ent(X), ent(A, stereo=1), ent(Y), ent(Z)]], want=dict(verdict=[R.CULLED], counts2=[[1, 1]]))
    # obs_kf_bad entries count (the reference does not ask isBad() of the observing keyframes)
    c["kf_bad_counts"] = case([red(A)], kf_bad=[0, 1, 1, 1], want=dict(verdict=[R.CULLED], counts2=[[1, 1]]))
    # the depth gate: == th counts, just above and < 0 do not; monocular ignores it
    for name, d, mono, counted in (("depth_at_th", TH, 0, 1), ("depth_above_th", ABOVE_TH, 0, 0), ("depth_negative", -1.0, 0, 0),
                                   ("depth_above_th_mono", ABOVE_TH, 1, 1), ("depth_negative_mono", -1.0, 1, 1)):
        c[name] = case([red(A, depth=d)], mono=mono, want=dict(verdict=[R.CULLED if counted else R.KEPT], counts2=[[counted, counted]]))
    # mnId == 0 and its twin
    c["id0"] = case([red(A)], flags=[1], want=dict(verdict=[R.SKIPPED_ID0], counts2=[[0, 0]], obs_dead=[0, 0, 0, 0]))
    # mbNotErase: the test passes, nothing is erased, so B still sees the shared points; the twin cascades
    shared = [red(A)] * 30 + [[ent(A), ent(B), ent(X)]] * 2 + [red(B)] * 10
    c["not_erase"] = case(shared, cand=(A, B), flags=[2, 0], want=dict(verdict=[R.TO_BE_ERASED, R.KEPT], counts2=[[30, 32], [10, 12]],
                                                                      info8=[0, 0, 1, 0, 0, 0, 0, 0]))
    c["cascade_A_B"] = cascade((A, B))
    c["cascade_B_A"] = cascade((B, A))
    # ref_obs moves to the first survivor; a list that empties
    c["ref_moves"] = case([[ent(X), ent(A), ent(Y), ent(Z), ent(W)], [ent(A), ent(X), ent(Y), ent(Z), ent(W)]], ref_obs=[1, 0],
                          want=dict(verdict=[R.CULLED], ref_obs=[0, 1], obs_dead=[0, 1, 0, 0, 0, 1, 0, 0, 0, 0], n_obs=[4, 4], point_bad=[0, 0]))
    c["list_empties"] = case([red(A)] * 20 + [[ent(A)], [ent(A), ent(X)]],
                             want=dict(verdict=[R.CULLED], counts2=[[20, 22]], ref_obs=[1] * 20 + [-1, 1], n_obs=[3] * 20 + [0, 1],
                                       point_bad=[0] * 20 + [1, 1], obs_dead=[1, 0, 0, 0] * 20 + [1, 1, 2]))
    # both refusals, and their twins on a bad point (whose entries are nobody's)
    c["not_resident"] = case([red(A), [ent(A), ent(-2), ent(Y), ent(Z)]], want=dict(info8=[R.NOT_RESIDENT, 0, 0, 0, 0, 0, 0, 0]))
    c["not_resident_bad_point"] = case([red(A), [ent(A), ent(-2), ent(Y), ent(Z)]], point_bad=[0, 1],
                                       want=dict(verdict=[R.CULLED], counts2=[[1, 1]], info8=[0, 1, 0, 1, 0, 0, 0, 0]))
    c["bad_index"] = case([red(A), [ent(A), ent(9), ent(Y), ent(Z)]], want=dict(info8=[R.BAD_INDEX, 0, 0, 0, 0, 0, 0, 0]))
    c["bad_index_bad_point"] = case([red(A), [ent(A), ent(-3), ent(Y), ent(Z)]], point_bad=[0, 1],
                                    want=dict(verdict=[R.CULLED], counts2=[[1, 1]]))
    # 0, 1 and 33 candidates: keyframe k of 36 sees point k redundantly; every third is flagged mnId == 0 / mbNotErase in turn
    c["no_candidates"] = case([red(A)], cand=(), want=dict(info8=[0] * 8, obs_dead=[0, 0, 0, 0]))
    pts33 = [[ent(k), ent(33), ent(34), ent(35)] for k in range(33)]
    fl33 = [(0, 1, 2)[k % 3] for k in range(33)]
    c["candidates_33"] = case(pts33, cand=tuple(range(33)), flags=fl33, n_kf=36,
                              want=dict(verdict=[(R.CULLED, R.SKIPPED_ID0, R.TO_BE_ERASED)[k % 3] for k in range(33)],
                                        info8=[0, 11, 11, 11, 0, 0, 0, 0]))
    # the current keyframe (-1) is a bystander like any other
    c["current_keyframe_counts"] = case([[ent(A), ent(R.CUR), ent(X), ent(Y)]], want=dict(verdict=[R.CULLED], counts2=[[1, 1]]))
    for P in (1, 1023, 1024, 1025):
        c[f"points_{P}"] = sized(P)
    return c


def random_map(seed, n_kf=24, n_points=600, lo=3, hi=12, n_cand=None):
    """A seeded map: every point is seen by lo .. hi keyframes (the current one among them now and then), mono and stereo mixed,
    octaves 0 .. 2, depths around the threshold, a few bad points; the candidates are a random order of most keyframes."""
    rng = np.random.default_rng(seed)
    pts = []
    for _ in range(n_points):
        k = int(rng.integers(lo, hi + 1))
        kfs = [int(v) for v in rng.choice(n_kf + 1, size=min(k, n_kf + 1), replace=False)]
        pts.append([ent(v if v < n_kf else R.CUR, int(rng.integers(0, 3)), int(rng.uniform() < 0.4), float(np.float32(rng.uniform(-5, 60))))
                    for v in kfs])
    ref = [int(rng.integers(0, len(o))) for o in pts]
    bad = (rng.uniform(size=n_points) < 0.03).astype(np.uint8)
    kf_bad = (rng.uniform(size=sum(len(o) for o in pts)) < 0.05).astype(np.uint8)
    n_cand = n_kf - 2 if n_cand is None else n_cand
    cand = rng.permutation(n_kf)[:n_cand]
    flags = rng.choice([0, 0, 0, 0, 1, 2], size=n_cand)
    return case(pts, cand=tuple(int(v) for v in cand), flags=[int(v) for v in flags], n_kf=n_kf, ref_obs=ref, point_bad=bad, kf_bad=kf_bad,
                mono=int(seed % 2))


def erase_cases():
    """name -> (problem, obs_erase, want): the hand cases of sd_debug_erase_observations.  Points 0 and 2 are bystanders."""
    by = [ent(X), ent(Y), ent(Z)]
    c = {}

    def one(name, point, erase, want, **kw):
        pts = [by, point, by]
        flags = [0] * 3 + list(erase) + [0] * 3
        c[name] = (R.problem(pts, 6, **kw), np.array(flags, np.uint8), want)

    four = [ent(A), ent(X), ent(Y), ent(Z)]
    one("leaves_3", four, [0, 1, 0, 0], dict(obs_off=[0, 3, 6, 9], obs_map=[0, 1, 2, 3, -1, 4, 5, 6, 7, 8], point_bad=[0, 0, 0], n_obs=[3, 3, 3]))
    one("leaves_2", lone(A), [0, 1, 0], dict(obs_off=[0, 3, 3, 6], obs_map=[0, 1, 2, -1, -1, -1, 3, 4, 5], point_bad=[0, 1, 0], n_obs=[3, 0, 3],
                                             ref_obs=[0, 0, 0]))
    one("stereo_entry", [ent(A, stereo=1), ent(X), ent(Y), ent(Z)], [1, 0, 0, 0],
        dict(obs_off=[0, 3, 6, 9], point_bad=[0, 0, 0], n_obs=[3, 3, 3]))
    one("stereo_entry_twin", [ent(A, stereo=1), ent(X), ent(Y)], [1, 0, 0], dict(obs_off=[0, 3, 3, 6], point_bad=[0, 1, 0], n_obs=[3, 0, 3]))
    one("ref_entry", [ent(A), ent(X), ent(Y), ent(Z), ent(W)], [0, 0, 1, 0, 0], dict(obs_off=[0, 3, 7, 10], ref_obs=[0, 0, 0], n_obs=[3, 4, 3]),
        ref_obs=[0, 2, 0])
    one("ref_entry_twin", [ent(A), ent(X), ent(Y), ent(Z), ent(W)], [0, 1, 0, 0, 0], dict(obs_off=[0, 3, 7, 10], ref_obs=[0, 1, 0]),
        ref_obs=[0, 2, 0])
    one("every_entry", four, [1, 1, 1, 1], dict(obs_off=[0, 3, 3, 6], point_bad=[0, 1, 0], n_obs=[3, 0, 3], info8=[0, 4, 1, 6, 0, 0, 0, 0]))
    one("nothing", four, [0, 0, 0, 0], dict(obs_off=[0, 3, 7, 10], obs_map=list(range(10)), point_bad=[0, 0, 0], ref_obs=[0, 1, 0],
                                            n_obs=[3, 4, 3], info8=[0, 0, 0, 10, 0, 0, 0, 0]), ref_obs=[0, 1, 0])
    one("bad_point_is_left_alone", lone(A), [0, 1, 0], dict(obs_off=[0, 3, 6, 9], point_bad=[0, 1, 0], info8=[0, 0, 0, 9, 0, 0, 0, 0]),
        point_bad=[0, 1, 0])
    return c
