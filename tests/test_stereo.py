"""Stereo / RGB-D depth on the device: uh_stereo_depth and its _dev twin against the numpy restatement of FrameExtractor::processStereo
(tests/stereo_oracle.py) bit for bit on the constructed scenes of tests/stereo_cases.py; uh_orb_extract_stereo / uh_orb_extract_rgbd against
the monocular extraction (byte-equal left and right outputs, the same device frame) and against the oracle run on those outputs; the returned
depth through uh_track_pose_stereo; the argument checks."""
import numpy as np
import pytest

import stereo_cases as SC
import stereo_oracle as O
import synth

BL, MDD = 0.54, 50.0
CAM = (718.856, 718.856, 607.19, 185.22)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, build in SC.CASES.items():
        out[name] = [(sc,) + O.stereo_depth(sc["L"], sc["R"], sc["lk"], sc["ld"], sc["rk"], sc["rd"], sc["bl"], sc["fx"], sc["mdd"]) for sc in build()]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.CASES))
def test_stereo_depth_equals_the_oracle_bit_for_bit(hip_ctx, solved, name):
    import torch

    from ucoslam_cv3_amd.stereo import stereo_depth, stereo_depth_dev

    for k, (sc, d, m) in enumerate(solved[name]):
        gd, gm = stereo_depth(hip_ctx, sc["L"], sc["R"], sc["lk"], sc["ld"], sc["rk"], sc["rd"], sc["bl"], sc["fx"], sc["mdd"])
        assert np.array_equal(gm, m), (name, k, gm.tolist()[:16], m.tolist()[:16])
        assert np.array_equal(bits(gd), bits(d)), (name, k, gd.tolist()[:16], d.tolist()[:16])
        # the _dev twin: everything resident, keypoints as the 28-byte records
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        rec = lambda a: t(np.ascontiguousarray(a).view(np.uint8).reshape(-1, 28))   # noqa: E731
        for want_match in (True, False):
            dd, dm = stereo_depth_dev(hip_ctx, t(sc["L"]), t(sc["R"]), rec(sc["lk"]), t(sc["ld"]), rec(sc["rk"]), t(sc["rd"]), sc["bl"], sc["fx"], sc["mdd"],
                                      want_match=want_match)
            hip_ctx.synchronize()
            assert np.array_equal(bits(dd.cpu().numpy()), bits(d)), (name, k, "dev", want_match)
            assert dm is None or np.array_equal(dm.cpu().numpy(), m)


@pytest.mark.gpu
def test_rgbd_depth_equals_the_oracle_bit_for_bit(hip_ctx):
    from ucoslam_cv3_amd.stereo import rgbd_depth

    k, D, scale = SC.rgbd_scene()
    want = O.rgbd_depth(k, D, scale)
    assert np.array_equal(bits(rgbd_depth(hip_ctx, k, D, scale)), bits(want))
    wide = np.zeros((SC.ROWS, SC.COLS + 6), np.uint16)
    wide[:, :SC.COLS] = D
    assert np.array_equal(bits(rgbd_depth(hip_ctx, k, wide[:, :SC.COLS], scale)), bits(want))
    assert len(rgbd_depth(hip_ctx, k[:0], D, scale)) == 0


def _extractor(hip_ctx, nf, nl, dist=(-1e-4, 0.0, 0.0, 0.0)):
    """the stereo default: a rectified pair, with just enough distortion left that und_kpts differ from kpts in their last bits"""
    from ucoslam_cv3_amd.orb import Camera, FeatParams, ORBextractor
    from ucoslam_cv3_amd.stereo import set_stereo

    ext = ORBextractor(hip_ctx)
    fp = FeatParams(maxFeatures=nf, nOctaveLevels=nl, scaleFactor=1.2)
    ext.setCamera(Camera(*CAM, dist))
    set_stereo(ext, BL, MDD)
    ext.detectAndCompute(np.zeros((0, 0), np.uint8), None, fp)   # (sets the parameters)
    return ext


def _tree_equal(a, b):
    assert a["depth"] == b["depth"] and a["root_box"].tobytes() == b["root_box"].tobytes()
    for k in ("nodes", "leaf_idx", "leaf_xy", "leaf_octave"):
        assert a[k].tobytes() == b[k].tobytes(), k


SIZES = [(160, 120, 500, 4, 5), (1241, 376, 2000, 8, 12)]


@pytest.fixture(scope="module")
def pairs():
    """(w, h) -> (left, right): the synthetic scene and the same scene `disparity` pixels further left with other noise"""
    return {(w, h): (synth.frame(w, h, seed=5), synth.frame(w, h, seed=6, shift=(disp, 0))) for (w, h, _nf, _nl, disp) in SIZES}


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_extract_stereo_is_the_monocular_extraction_plus_the_oracles_depth(hip_ctx, pairs, size):
    from ucoslam_cv3_amd.orb import DeviceFrame
    from ucoslam_cv3_amd.stereo import extract_stereo

    w, h, nf, nl, _disp = size
    left, right = pairs[(w, h)]
    ext = _extractor(hip_ctx, nf, nl)
    kps, desc, und = ext.extractFrame(left)
    rk, rd = ext.detectAndCompute(right)
    fr_mono = DeviceFrame(hip_ctx)
    ext.extractFrameDev(left, fr_mono)
    tree_mono = fr_mono.tree()
    assert len(kps) > 50 and len(rk) > 50
    ukp = kps.copy()
    ukp["x"], ukp["y"] = und[:, 0], und[:, 1]
    want_d, want_m = O.stereo_depth(left, right, ukp, desc, rk, rd, BL, CAM[0], MDD)
    share = float((want_d != 0).mean())
    print(f"{w} x {h}: {len(kps)} left / {len(rk)} right keypoints, {int((want_m >= 0).sum())} matched, share with a depth {share:.3f}")
    assert share > 0.2   # (of the oracle alone: the comparison below is not an empty one)
    for frame in (None, DeviceFrame(hip_ctx)):
        for img_l, img_r in ((left, right), (np.stack([left] * 3, -1), np.stack([right] * 3, -1))):   # gray; BGR with equal channels: the same gray
            if img_l.ndim == 3:
                k3, d3, u3 = ext.extractFrame(img_l)
                assert k3.tobytes() == kps.tobytes()   # (so the gray expectations hold for the colour call)
            r = extract_stereo(ext, img_l, img_r, frame=frame, want_right=True)
            assert r["kps"].tobytes() == kps.tobytes() and r["desc"].tobytes() == desc.tobytes() and r["und_xy"].tobytes() == und.tobytes()
            assert r["right_kps"].tobytes() == rk.tobytes() and r["right_desc"].tobytes() == rd.tobytes()
            assert np.array_equal(bits(r["depth"]), bits(want_d))
            if frame is not None:
                _tree_equal(frame.tree(), tree_mono)
    r = extract_stereo(ext, left, right)   # without the inspection output
    assert np.array_equal(bits(r["depth"]), bits(want_d)) and r["kps"].tobytes() == kps.tobytes()
    # the monocular call is unchanged behind a stereo one
    k2, d2, u2 = ext.extractFrame(left)
    assert k2.tobytes() == kps.tobytes() and d2.tobytes() == desc.tobytes() and u2.tobytes() == und.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_extract_rgbd_is_the_monocular_extraction_plus_the_oracles_depth(hip_ctx, pairs, size):
    from ucoslam_cv3_amd.orb import DeviceFrame
    from ucoslam_cv3_amd.stereo import extract_rgbd

    w, h, nf, nl, _disp = size
    img = pairs[(w, h)][0]
    rng = np.random.default_rng(41)
    D = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    D[rng.random((h, w)) < 0.3] = 0
    scale = np.float32(1.0 / 5000.0)
    ext = _extractor(hip_ctx, nf, nl, dist=(-0.05, 0.01, 0.001, -0.001))   # (the gather reads the DISTORTED keypoints)
    kps, desc, und = ext.extractFrame(img)
    fr_mono = DeviceFrame(hip_ctx)
    ext.extractFrameDev(img, fr_mono)
    want = O.rgbd_depth(kps, D, scale)
    assert 0.5 < float((want != 0).mean()) < 0.9
    for frame in (None, DeviceFrame(hip_ctx)):
        r = extract_rgbd(ext, img, D, scale, frame=frame)
        assert r["kps"].tobytes() == kps.tobytes() and r["desc"].tobytes() == desc.tobytes() and r["und_xy"].tobytes() == und.tobytes()
        assert np.array_equal(bits(r["depth"]), bits(want))
        if frame is not None:
            _tree_equal(frame.tree(), fr_mono.tree())
    r = extract_rgbd(ext, img, D, scale, undistorted=False)
    assert np.array_equal(bits(r["depth"]), bits(want)) and r["und_xy"] is None


@pytest.mark.gpu
def test_track_pose_stereo_fed_with_the_returned_depth(hip_ctx):
    """uh_orb_extract_stereo -> uh_track_pose_stereo: the tracker's result with the device's depth array is its result with the oracle's."""
    from test_track import _same, _scene

    from ucoslam_cv3_amd.pnp import PnPSolver
    from ucoslam_cv3_amd.stereo import extract_stereo, set_stereo

    sc = _scene(hip_ctx, 5, False)
    ext, fr = sc["keep"]
    left, right = synth.frame(1241, 376, seed=5), synth.frame(1241, 376, seed=6, shift=(12, 0))
    set_stereo(ext, BL, MDD)
    r = extract_stereo(ext, left, right, frame=fr, want_right=True)
    assert r["und_xy"].tobytes() == sc["und"].tobytes()   # the scene's own frame again
    sc["pm"].setFrameDev(fr, np.cumprod(np.concatenate([[np.float32(1)], np.full(7, np.float32(1.2))]).astype(np.float32)).astype(np.float32),
                         sc["intr"][0], sc["intr"][1], sc["intr"][2], sc["intr"][3], (0, 0), (1241, 376), und_kpts=sc["ukp"])
    want_d, _ = O.stereo_depth(left, right, sc["ukp"], r["desc"], r["right_kps"], r["right_desc"], BL, float(sc["intr"][0]), MDD)
    assert (want_d > 0).mean() > 0.2
    pnp = PnPSolver(hip_ctx)
    kw = dict(prev_map_row=sc["prev_row"], map_weight=sc["weight"], bl=BL)
    got = sc["pm"].trackPoseStereo(pnp, sc["pose0"], sc["intr"], sc["inv_sf"], sc["prev"], sc["mp"], depth=r["depth"], **kw)
    want = sc["pm"].trackPoseStereo(pnp, sc["pose0"], sc["intr"], sc["inv_sf"], sc["prev"], sc["mp"], depth=want_d, **kw)
    _same(got, want, "device depth against oracle depth")
    assert got["tracked"]


@pytest.mark.gpu
def test_argument_checks_return_before_any_launch(hip_ctx):
    from ucoslam_cv3_amd import UcoslamHipError
    from ucoslam_cv3_amd._lib import UH_EINVAL
    from ucoslam_cv3_amd.orb import FeatParams, ORBextractor
    from ucoslam_cv3_amd.stereo import extract_stereo, set_stereo, stereo_depth

    sc = SC.equal_hamming()[0]
    args = [sc["L"], sc["R"], sc["lk"], sc["ld"], sc["rk"], sc["rd"], sc["bl"], sc["fx"], sc["mdd"]]
    hip_ctx.prof_enable(True)
    hip_ctx.prof_reset()
    try:
        with pytest.raises(UcoslamHipError, match="uh_stereo_depth: left image 64 x 48 but right image 64 x 47") as e:
            stereo_depth(hip_ctx, sc["L"], sc["R"][:47], *args[2:])
        assert e.value.code == UH_EINVAL
        for bl in (0.0, -0.54):   # with a match in the scene
            with pytest.raises(UcoslamHipError, match="uh_stereo_depth: baseline") as e:
                stereo_depth(hip_ctx, *args[:6], bl, sc["fx"], sc["mdd"])
            assert e.value.code == UH_EINVAL
        with pytest.raises(UcoslamHipError, match="uh_stereo_depth: keypoint counts"):
            stereo_depth(hip_ctx, *args, n_right=(1 << 24) + 1)
        ext = ORBextractor(hip_ctx)
        ext.detectAndCompute(np.zeros((0, 0), np.uint8), None, FeatParams(500, 4, 1.2))
        img = synth.frame(160, 120, seed=1)
        with pytest.raises(UcoslamHipError, match="uh_orb_extract_stereo: no camera set"):
            extract_stereo(ext, img, img)
        with pytest.raises(UcoslamHipError, match="uh_orb_set_stereo: baseline"):
            set_stereo(ext, 0.0, MDD)
        with pytest.raises(UcoslamHipError, match="left image .* but right image"):
            extract_stereo(ext, img, img[:100])
        assert hip_ctx.prof_report() == {}   # nothing was launched
    finally:
        hip_ctx.prof_enable(False)
    # over capacity: the count comes back with UH_ECAPACITY, as from uh_orb_extract_frame
    from ucoslam_cv3_amd._lib import UH_ECAPACITY
    from ucoslam_cv3_amd.orb import Camera

    ext.setCamera(Camera(*CAM, ()))
    set_stereo(ext, BL, MDD)
    with pytest.raises(UcoslamHipError, match="capacity 10") as e:
        extract_stereo(ext, img, img, cap=10)
    assert e.value.code == UH_ECAPACITY
