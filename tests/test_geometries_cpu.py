"""The oracle and numpy alone at the frame geometries of tests/geometries.py: the cases tests/test_geometries_gpu.py runs are
sound (the extraction plan accepts every frame size and its level sizes are the oracle's; the extractor finds its keypoints;
ImageAlign converges; the searches find their matches; TrackWithMotionModel and TrackLocalMap track; the planted border points
lie where they claim; every aligned level sees enough points), and the sweep has teeth: with VGA bounds, with the depth map
read at [u, v] or with stride W, or with cols and rows exchanged in ImageAlign's clip test, the oracle or the numpy restatement
gives something else than the right thing in a quantity the GPU file asserts.  One test, test_the_plan_accepts_every_geometry,
also calls the host-only sd_orb_plan_info of the built library (no GPU needed, but the library has to be built)."""
import numpy as np
import pytest

import cameras as CM
import geometries as G

VGA_BOUNDS = (0.0, 640.0, 0.0, 480.0)
MIN_KEYPOINTS, MIN_MATCHES, MIN_INLIERS, MIN_VISIBLE = 150, 60, 30, 8       # conditions on the cases, not measurements


def _log_sf(geo):
    return np.log(np.float32(geo.cfg[1]))


def _align(O, rig, i, mode=0, cur=None, ref=None):
    """ImageAlign as the GPU file calls it: modes 0 and 1 on `last` (300 points), mode 3 on `last3` (100 points)."""
    f, s = rig["fr"][i], rig["scenes"][i]
    last = f["last3"] if mode == 3 else f["last"]
    return O.align(f["pc"] if cur is None else cur, f["pr"] if ref is None else ref, f["tab"]["inv_sf"], f["tab"]["sf"], G.align_points(last),
                   s["T_ref"], CM.START @ s["T_cur"], rig["cam"].K, mode=mode)


def _match(O, rig, i, T, bounds=None, th=8.0):
    f, s, cam = rig["fr"][i], rig["scenes"][i], rig["cam"]
    return O.search_by_projection(f["ck"], f["cd"], f["tab"]["sf"], cam.bounds if bounds is None else bounds, cam.K, T, s["T_ref"], f["last"], th=th,
                                  mono=True, check_ori=True)


def _local(O, rig, i, bounds=None):
    f, s, cam = rig["fr"][i], rig["scenes"][i], rig["cam"]
    return O.search_local_points(f["ck"], f["cd"], f["tab"]["sf"], _log_sf(rig["geo"]), cam.bounds if bounds is None else bounds, cam.K, 0.0, s["T_cur"],
                                 f["local"], th=1.0, nnratio=0.8)


def _area(O, rig, i, bounds=None):
    return [O.features_in_area(rig["fr"][i]["ck"], rig["cam"].bounds if bounds is None else bounds, *q) for q in G.area_queries(rig["geo"])]


def _track(O, rig, i, bounds=None):
    f, s, cam = rig["fr"][i], rig["scenes"][i], rig["cam"]
    b = cam.bounds if bounds is None else bounds
    tw = O.track_with_motion_model(f["pc"], f["pr"], f["tab"], f["ck"], f["cd"], b, cam.K, s["T_ref"], CM.START @ s["T_cur"], f["last"], 8.0, mono=True,
                                   align_mode=0)
    lm = O.track_local_map(f["ck"], f["cd"], f["tab"], _log_sf(rig["geo"]), b, cam.K, tw["T"], tw["match"], f["last"], f["local"], th=1.0, min_inliers=30)
    return tw, lm


def _depth(rig, i, which, **kw):
    """The restatement of k_stereo_from_depth on frame i's strided buffer; which = a row of G.DEPTH_CALLS."""
    tag, _, factor, convert = which
    geo, f = rig["geo"], rig["fr"][i]
    flat, stride, fstride = rig["buf_" + tag]
    args = dict(w=geo.w, h=geo.h, stride=stride, fstride=fstride)
    args.update(kw)
    return G.stereo_from_depth(f["ck"], f["ck"], flat, i, convert=convert, scale=G.depth_scale(factor), bf=G.BF, **args)


def _pose_err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_the_plan_accepts_every_geometry(oracle):
    """sd_orb_plan_info takes each frame size as it stands in the table, and its level sizes are the oracle's level(l) shapes."""
    from sdslam_amd import capi
    for name in G.NAMES:
        geo, rig = G.GEOMETRIES[name], G.oracle_rig(oracle, name)
        lv = capi.plan_info(*geo.cfg, geo.w, geo.h)["levels"]
        assert [(int(h), int(w)) for w, h in lv[:, :2]] == [tuple(s) for s in rig["fr"][0]["shapes"]], name
    sh = G.oracle_rig(oracle, "small15")["fr"][0]["shapes"]
    assert sh[4] == (48, 63)
    assert all(r > c for r, c in G.oracle_rig(oracle, "portrait")["fr"][0]["shapes"])


@pytest.mark.parametrize("name", G.NAMES)
def test_cases_are_sound(oracle, name):
    rig = G.oracle_rig(oracle, name)
    geo, cam = rig["geo"], rig["cam"]
    print(f"\n{name} {geo.w} x {geo.h}: frame, keypoints cur / ref, align error mode 0 / 1, frame matches th 8, map matches, local-map inliers")
    for i in range(rig["B"]):
        f, s = rig["fr"][i], rig["scenes"][i]
        assert len(f["ck"]) >= MIN_KEYPOINTS and len(f["rk"]) >= MIN_KEYPOINTS, (name, i, len(f["ck"]), len(f["rk"]))
        assert len(f["ck"]) <= geo.cfg[0] and len(f["last"]["valid"]) <= G.MP and len(f["local"]["cand"]) <= G.MP
        assert f["last"]["valid"].sum() == G.N_ALIGNED and f["last"]["valid"][-G.N_PLANTED:].all()       # ImageAlign reads every planted point
        errs = []
        for mode in (0, 1):
            al = _align(oracle, rig, i, mode)
            assert al["ok"], (name, i, mode)
            errs.append(CM.pose_close(al["T"], s["T_cur"], (name, i, mode)))
        assert _align(oracle, rig, i, 3)["ok"], (name, i, 3)
        v3 = f["last3"]["valid"]
        assert v3.sum() == G.N_ALIGNED_KF and v3[-len(f["Xp3"]):].all()              # mode 3 reads every point planted for it
        nm, _ = _match(oracle, rig, i, _align(oracle, rig, i)["T"])
        assert nm >= MIN_MATCHES, (name, i, nm)
        tw, lm = _track(oracle, rig, i)
        assert tw["status"] == 2 and lm["n_inliers"] >= MIN_INLIERS and lm["status"] == 2, (name, i, tw["status"], lm["n_inliers"])
        print(f"  {i}  {len(f['ck'])} / {len(f['rk'])}  {errs[0]:.2e} / {errs[1]:.2e}  {nm}  {tw['nmatches_map']}  {lm['n_inliers']}")
        # the depth maps give most keypoints a depth, leave some without, and carry no poison
        for which in G.DEPTH_CALLS:
            ur, dd = _depth(rig, i, which)
            assert (dd > 0).sum() >= 100 and (dd < 0).sum() >= 10, (name, i, which)
            poison = np.float32(G.POISON_F32 if which[0] == "f32" else G.POISON_U16) * (G.depth_scale(which[2]) if which[3] else np.float32(1))
            assert not (dd == poison).any() and (dd < 20.0 * 5000.0).all(), (name, i, which)
        area = _area(oracle, rig, i)
        assert sum(len(a) for a in area) > 100 and sum(len(a) for a in area[:7]) >= 10 and len(area[4]) + len(area[6]) > 0 and \
            len(area[5]) + len(area[6]) > 0, (name, i, [len(a) for a in area])      # lists at the right and at the bottom bound are not empty
        x, y = f["ck"]["x"], f["ck"]["y"]
        if name == "wide":
            assert (x > 640).sum() >= 10, (i, (x > 640).sum())
        if name == "portrait":
            assert (y > 480).sum() >= 10 and (y > x).sum() >= 50, (i, (y > 480).sum())


@pytest.mark.parametrize("name", G.NAMES)
def test_planted_points_are_what_they_claim(oracle, name):
    """By the clip restatement at T_ref: each pair lands on its two sides of its level's limit, half a level pixel from it; every
    aligned level has at least 8 visible points; in portrait, wide and small15 a planted point of every level changes sides when
    cols and rows are exchanged; in odd one changes sides when the level size is truncated instead of rounded.  The same for
    mode 3's own last frame: its four level-4 points under the scale (float)(1.0 / sf[4]), among its 100 points."""
    rig = G.oracle_rig(oracle, name)
    geo, K = rig["geo"], rig["cam"].K
    for i in range(rig["B"]):
        f, T_ref = rig["fr"][i], rig["scenes"][i]["T_ref"]
        inv_sf, flipped_swap, flipped_trunc = f["tab"]["inv_sf"], set(), set()
        for k, (l, axis, visible) in enumerate(f["claims"]):
            rows, cols = f["shapes"][l]
            P = f["Xp"][k:k + 1]
            uf, vf, behind = G.project_level(P, T_ref, K, inv_sf[l])
            at, n = (uf[0], cols) if axis == 0 else (vf[0], rows)
            assert not behind[0] and at + 3 == (n - 1 if visible else n), (name, i, k, at, n)
            assert G.clip_visible(P, T_ref, K, inv_sf[l], cols, rows)[0] == visible, (name, i, k)
            if G.clip_visible(P, T_ref, K, inv_sf[l], rows, cols)[0] != visible:
                flipped_swap.add(l)
            tc, tr = int(geo.w * np.float32(inv_sf[l])), int(geo.h * np.float32(inv_sf[l]))
            if G.clip_visible(P, T_ref, K, inv_sf[l], tc, tr)[0] != visible:
                flipped_trunc.add(l)
        if name in ("portrait", "wide", "small15"):
            assert flipped_swap == set(G.ALIGNED_LEVELS), (name, i, flipped_swap)
        if name == "odd":
            assert flipped_trunc, (name, i)
            assert any((int(geo.w * np.float32(inv_sf[l])), int(geo.h * np.float32(inv_sf[l]))) != f["shapes"][l][::-1] for l in G.ALIGNED_LEVELS)
        for l in G.ALIGNED_LEVELS:
            rows, cols = f["shapes"][l]
            n_vis = int(G.clip_visible(G.align_points(f["last"]), T_ref, K, inv_sf[l], cols, rows).sum())
            assert n_vis >= MIN_VISIBLE, (name, i, l, n_vis)
        # mode 3: level 4 alone, the first 100 valid points, scale (float)(1.0 / sf[4])
        s3, (rows, cols) = G.kf_scale(f["tab"]["sf"]), f["shapes"][4]
        P3 = G.align_points(f["last3"])
        assert len(P3) == G.N_ALIGNED_KF and np.array_equal(P3[-4:], f["Xp3"]) and [c[0] for c in f["claims3"]] == [4] * 4
        swap3 = trunc3 = 0
        for k, (l, axis, visible) in enumerate(f["claims3"]):
            P = f["Xp3"][k:k + 1]
            uf, vf, behind = G.project_level(P, T_ref, K, s3)
            at, n = (uf[0], cols) if axis == 0 else (vf[0], rows)
            assert not behind[0] and at + 3 == (n - 1 if visible else n), (name, i, "mode 3", k, at, n)
            assert G.clip_visible(P, T_ref, K, s3, cols, rows)[0] == visible, (name, i, "mode 3", k)
            swap3 += G.clip_visible(P, T_ref, K, s3, rows, cols)[0] != visible
            trunc3 += G.clip_visible(P, T_ref, K, s3, int(geo.w * s3), int(geo.h * s3))[0] != visible
        if name in ("portrait", "wide", "small15"):
            assert swap3 > 0, (name, i, "mode 3")
        if name == "odd":
            assert trunc3 > 0, (name, i, "mode 3")
        n_vis = int(G.clip_visible(P3, T_ref, K, s3, cols, rows).sum())
        assert n_vis >= MIN_VISIBLE, (name, i, "mode 3", n_vis)


def _align_differs(a, b):
    return (a["ok"] != b["ok"] or not np.array_equal(a["iters"], b["iters"]) or _pose_err(a["T"], b["T"]) > 1e-5
            or abs(a["error"] - b["error"]) > 1e-7 * max(1.0, abs(a["error"])))


def _differs(O, rig):
    """mutation -> {quantity the GPU file asserts: differs from the right one on frame 0}."""
    i, geo = 0, rig["geo"]
    f = rig["fr"][i]
    out = {}
    if rig["cam"].bounds != VGA_BOUNDS:
        T = rig["scenes"][i]["T_cur"]
        a, b = _local(O, rig, i), _local(O, rig, i, VGA_BOUNDS)
        (ta, la), (tb, lb) = _track(O, rig, i), _track(O, rig, i, VGA_BOUNDS)
        out["VGA bounds"] = {
            "match": any(not np.array_equal(_match(O, rig, i, T, th=th)[1], _match(O, rig, i, T, VGA_BOUNDS, th=th)[1]) for th in (8.0, 1.0)),
            "match_local": any(not np.array_equal(a[k], b[k]) for k in ("match", "in_view", "level", "proj")),
            "features_in_area": any(not np.array_equal(x, y) for x, y in zip(_area(O, rig, i), _area(O, rig, i, VGA_BOUNDS))),
            "grid": not np.array_equal(G.grid_occupancy(f["ck"], rig["cam"].bounds), G.grid_occupancy(f["ck"], VGA_BOUNDS)),
            "track": not np.array_equal(ta["match"], tb["match"]) or not np.array_equal(la["local_match"], lb["local_match"])}
    right = {w: _depth(rig, i, w) for w in G.DEPTH_CALLS}
    out["depth [u, v]"] = {"stereo " + w[0] + " x %g" % w[2]: not all(np.array_equal(x, y) for x, y in zip(right[w], _depth(rig, i, w, swap_uv=True)))
                           for w in G.DEPTH_CALLS}
    out["depth stride W"] = {"stereo " + w[0] + " x %g" % w[2]: not all(np.array_equal(x, y) for x, y in zip(right[w], _depth(rig, i, w, stride=geo.w)))
                             for w in G.DEPTH_CALLS}
    # This row shows that exchanged cols / rows reach the aligner's results at all: the exchanged shape clips every ordinary point
    # beyond min(rows, cols), at vga too, so it says nothing about the planted points or about a size.  That a device with the
    # two exchanged would be caught by the PLANTED points, at the sizes where nothing else shows it, is what
    # test_planted_points_are_what_they_claim asserts (flipped_swap per level, swap3 for mode 3).
    cur, ref = G.swapped_levels(f["pc"], f["pc_pad"], f["shapes"]), G.swapped_levels(f["pr"], f["pr_pad"], f["shapes"])
    for l in G.ALIGNED_LEVELS:          # the exchanged arrays hold the same pixels at the same pitch where the image is
        r, c = f["shapes"][l]
        m = min(r, c)
        assert np.array_equal(ref[l][:m, :m], f["pr"][l][:m, :m]) and ref[l].shape == (c, r)
    out["clip cols<->rows"] = {"align mode %d" % m: _align_differs(_align(O, rig, i, m), _align(O, rig, i, m, cur, ref)) for m in (0, 1, 3)}
    return out


@pytest.mark.parametrize("name", G.NAMES)
def test_every_mutation_is_detected(oracle, name):
    rig = G.oracle_rig(oracle, name)
    table = _differs(oracle, rig)
    print(f"\n{name}: mutation -> quantity: differs / same")
    for label, row in table.items():
        print(f"{label:>18}: " + ", ".join(f"{k} {'differs' if v else 'same'}" for k, v in row.items()))
    for label, row in table.items():
        assert any(row.values()), (name, label)
    assert ("VGA bounds" in table) == (name != "vga")
    # where the frame is not VGA, wrong bounds move the grid itself; and both depth mutations show under every call
    if name != "vga":
        assert table["VGA bounds"]["grid"] and table["VGA bounds"]["features_in_area"], name
    assert all(table["depth [u, v]"].values()) and all(table["depth stride W"].values()), name
