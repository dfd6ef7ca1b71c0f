"""GPU tests (-m gpu) of the flat-attribute shading event of the shipped build's LDS kernels (trg_kernels.hip shade_event FLAT): a scene whose
triangles each have ONE normal and ONE colour is shaded from one 48-byte record per triangle -- (unit normal | r) (right | g) (forward | b) --
instead of interpolating 18 floats and building the tangent frame per hit.  The bar is the shipped build's small-image bar against the oracle
(tests/util.py fast_bar: RMSE <= 1e-3, outlier pixels within edge_flip_allowance); where the generic kernel must run -- a smooth-shaded
triangle in the scene, a texture loaded -- the picture is the one TRG_FLAT_SHADING=0 gives, bit for bit.

Measured on an MI355X when the form was introduced (every test prints its figures, `pytest -s`): no outlier pixel in any case (8 - 10 allowed),
RMSE 5e-8 ... 1e-7 against the oracle; the Cornell box at 64 x 48, 4 spp differs from the image the same library gives with TRG_FLAT_SHADING=0
in 822 of 3,072 pixels (last-bit differences: RMSE against the oracle 9.50e-8 with the form, 9.49e-8 without)."""
import numpy as np
import pytest

from tests.util import fast_bar, make_ctx

pytestmark = pytest.mark.gpu

# Which of the three schedules' shipped-build images were bit-identical to each other on the PARENT commit (48 x 40, 4 spp, 5 bounces, measured
# there with these same renders): the frame-serial kernel and the frame-lane split were; head / tail differed from both in 32 of the 1,920
# pixels (another kernel: the compiler contracts its arithmetic differently).  The pair that was identical must stay so with the flat form on.
PARENT_IDENTICAL = {("serial", "frame_split"): True, ("serial", "head_tail"): False, ("frame_split", "head_tail"): False}


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _differing(a, b):
    return int((_bits(a) != _bits(b)).any(-1).sum())


def _render(capi, O, scene, w, h, spp, bnc, off, frame_split=1, tail=0, textures=None, parts=None):
    """The shipped build's image of `scene` and the rays it traced."""
    c = make_ctx(O, scene, w, h, offsets=off)
    try:
        if textures is not None:
            c.load_textures(*textures)
        c.set_option(capi.OPT_STRICT, 0)
        c.set_option(capi.OPT_FRAME_SPLIT, frame_split)
        c.set_option(capi.OPT_TAIL_BOUNCE, tail)
        c.reset_stats()
        for f0, n in (parts or ((0, spp),)):
            c.render(f0, n, bnc)
        return c.read_accum(), c.stats()
    finally:
        c.close()


def _is_flat(capi, scene):
    b = scene.buffers()
    return capi.debug_flat_attributes(b["normals"], b["colors"])[0]


def _assert_bar(tag, img, ref, rays):
    ok, rmse, outliers, allowed = fast_bar(img, ref, rays)
    print("%s: rmse %.3g, outlier pixels %d (allowed %d)" % (tag, rmse, outliers, allowed))
    assert ok, (tag, rmse, outliers, allowed)


def test_cornell_box_against_the_oracle(capi, O, cornell, monkeypatch):
    w, h, spp, bnc = 64, 48, 4, 3
    off = O.pixel_offsets(w, h)
    ref, rst = O.render(cornell, w, h, spp, bnc, offsets=off)
    monkeypatch.delenv("TRG_FLAT_SHADING", raising=False)
    assert _is_flat(capi, cornell)
    img, st = _render(capi, O, cornell, w, h, spp, bnc, off)
    assert st.scene_in_lds == 1
    _assert_bar("flat form on", img, ref, rst.rays)
    monkeypatch.setenv("TRG_FLAT_SHADING", "0")
    assert not _is_flat(capi, cornell)
    generic, _ = _render(capi, O, cornell, w, h, spp, bnc, off)
    _assert_bar("flat form off", generic, ref, rst.rays)
    print("pixels of %d that differ between the flat form and the generic one: %d" % (w * h, _differing(img, generic)))   # (reported, not asserted)


def test_schedules_agree(capi, O, cornell, monkeypatch):
    """Frame-serial kernel, frame-lane split and head / tail compaction at 48 x 40 (partial tiles), 5 bounces: each within the bar, and identical to
    each other wherever the parent commit's shipped build was (PARENT_IDENTICAL)."""
    w, h, spp, bnc = 48, 40, 4, 5
    off = O.pixel_offsets(w, h)
    ref, rst = O.render(cornell, w, h, spp, bnc, offsets=off)
    monkeypatch.delenv("TRG_FLAT_SHADING", raising=False)
    imgs = {}
    for name, kw in (("serial", {}), ("frame_split", {"frame_split": 2}), ("head_tail", {"tail": 2})):
        imgs[name], st = _render(capi, O, cornell, w, h, spp, bnc, off, **kw)
        if name == "frame_split":
            assert st.last_frame_split == 2
        if name == "head_tail":
            assert st.last_tail_bounce == 2
        _assert_bar(name, imgs[name], ref, rst.rays)
    for (a, b), identical in PARENT_IDENTICAL.items():
        n = _differing(imgs[a], imgs[b])
        print("%s vs %s: %d pixels differ" % (a, b, n))
        if identical:
            assert n == 0, (a, b, n)


def _flat_scene(O):
    """A tilted quad and a rotated, sheared cube under the default light: one normal of length 2 and one colour per triangle."""
    unit = O.OracleScene()
    unit.add("cube", (1.0, 1.0, 1.0), np.eye(4, dtype=np.float32))
    cube = unit.buffers()["positions"].reshape(-1, 3).astype(np.float64)          # addCube's 36 vertices
    c, s = np.cos(0.6), np.sin(0.6)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    shear = np.eye(3); shear[0, 1] = 0.5
    cube = cube @ (rot @ shear @ np.diag([0.3, 0.35, 0.25])).T + np.array([0.1, 0.7, -0.1])
    q = np.array([[-1.4, 1.3, -1.2], [1.4, 1.6, -1.2], [1.4, 0.3, 1.4], [-1.4, 0.0, 1.4]])       # tilted about x and about z
    quad = q[[0, 2, 1, 0, 3, 2]]
    pos = np.concatenate([quad, cube]).astype(np.float32)
    T = pos.reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    outward = np.concatenate([np.tile([0.0, 1.0, 0.0], (2, 1)), T[2:].mean(1) - cube.mean(0)])      # the quad faces up, the cube's faces away from its centre
    n *= np.sign((n * outward).sum(1, keepdims=True))
    n = 2.0 * n / np.linalg.norm(n, axis=1, keepdims=True)
    rng = np.random.default_rng(9)
    col = rng.uniform(0.2, 0.95, (T.shape[0], 3))
    scene = O.OracleScene()
    scene.add_raw(pos, np.repeat(n, 3, axis=0).astype(np.float32), np.repeat(col, 3, axis=0).astype(np.float32), np.ones(T.shape[0], np.uint32))
    return scene


def test_hand_made_flat_scene_against_the_oracle(capi, O, monkeypatch):
    w, h, spp, bnc = 64, 48, 4, 3
    scene = _flat_scene(O)
    monkeypatch.delenv("TRG_FLAT_SHADING", raising=False)
    assert _is_flat(capi, scene) and scene.ntris == 14
    off = O.pixel_offsets(w, h)
    ref, rst = O.render(scene, w, h, spp, bnc, offsets=off)
    assert (ref[..., :3].max(-1) > 0.01).mean() > 0.2 and rst.shaded_hits > 0.3 * w * h * spp      # the geometry is in the picture, and lit
    img, st = _render(capi, O, scene, w, h, spp, bnc, off)
    assert st.scene_in_lds == 1
    _assert_bar("tilted quad + sheared cube", img, ref, rst.rays)


def _smooth_scene(O):
    """The Cornell box and ONE triangle whose vertex normals differ."""
    s = O.OracleScene.cornell_box()
    pos = np.array([[-0.5, 0.9, 0.6], [0.3, 0.9, 0.6], [-0.1, 1.5, 0.4]], np.float32)
    nrm = np.array([[0.2, 0.1, 1.0], [-0.3, 0.0, 1.0], [0.0, 0.4, 1.0]], np.float32)
    s.add_raw(pos, nrm, np.full((3, 3), 0.7, np.float32), [1])
    return s


def _textured_wall(scene):
    """uvs, ids, images: an 8 x 8 checker on every triangle but the first cube's twelve."""
    n = scene.ntris
    uv = np.tile(np.array([[0, 0], [3, 0], [0, 3]], np.float32), (n, 1))
    ids = np.zeros(n, np.uint32)
    ids[12:] = 1
    img = np.zeros((8, 8, 4), np.uint8)
    img[..., 3] = 255
    img[::2, ::2, :3] = 240
    img[1::2, 1::2, :3] = 240
    img[..., 1] |= 30
    return uv, ids, [img]


@pytest.mark.parametrize("case", ["smooth_triangle", "texture_after_scene"])
def test_generic_kernel_where_the_flat_form_does_not_apply(capi, O, cornell, monkeypatch, case):
    w, h, spp, bnc = 64, 48, 3, 3
    off = O.pixel_offsets(w, h)
    monkeypatch.delenv("TRG_FLAT_SHADING", raising=False)
    if case == "smooth_triangle":
        scene, tex = _smooth_scene(O), None
        assert not _is_flat(capi, scene)
    else:
        scene, tex = cornell, _textured_wall(cornell)
        assert _is_flat(capi, scene)
    img, st = _render(capi, O, scene, w, h, spp, bnc, off, textures=tex)
    assert st.scene_in_lds == 1
    monkeypatch.setenv("TRG_FLAT_SHADING", "0")
    off_img, _ = _render(capi, O, scene, w, h, spp, bnc, off, textures=tex)
    assert np.array_equal(_bits(img), _bits(off_img)), _differing(img, off_img)
    if tex is not None:                   # the texture is in the picture: the flat records (which know nothing of it) were not used
        oscene = O.OracleScene.cornell_box()
        plain, _ = O.render(oscene, w, h, spp, bnc, offsets=off)
        oscene.set_textures(*tex)
        ref, rst = O.render(oscene, w, h, spp, bnc, offsets=off)
        assert (np.abs(ref[..., :3] - plain[..., :3]).max(-1) > 1e-2).mean() > 0.3
        _assert_bar("textured", img, ref, rst.rays)


def test_continued_average(capi, O, cornell, monkeypatch):
    """Frames [0, 8) in one launch and as [0, 4) + [4, 4): the same bits (the running average's arithmetic is one helper for every launch)."""
    w, h, bnc = 48, 40, 3
    off = O.pixel_offsets(w, h)
    monkeypatch.delenv("TRG_FLAT_SHADING", raising=False)
    whole, _ = _render(capi, O, cornell, w, h, 8, bnc, off)
    split, _ = _render(capi, O, cornell, w, h, 8, bnc, off, parts=((0, 4), (4, 4)))
    assert np.array_equal(_bits(whole), _bits(split)), _differing(whole, split)
    ref, rst = O.render(cornell, w, h, 8, bnc, offsets=off)
    _assert_bar("8 frames", whole, ref, rst.rays)
