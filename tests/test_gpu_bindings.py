"""GPU tests (-m gpu) of what the pose, skin and morph units SHARE (the binding of toyraygun_amd/csrc/trg_refit.hip; DESIGN.md, "Bindings"): the
three bound on ONE context keep their own copies, their own current and previous pose and their own release, and the loaded scene is the last
apply's.  Scene A, indexed (706 triangles, 424 vertices), on the host-built tree; the inputs are those of the units' own tests, so every box and
quad leaf survives every apply.  Images 32 x 24, 2 spp, 3 bounces; traces 4,096 random rays.  Nothing here provokes a fault: the one refused call
is decided on the host before anything is enqueued."""
import numpy as np
import pytest

from tests import morph_scenes as MS
from tests import pose_scenes as PS
from tests import refit_scenes as RS
from tests import skin_scenes as SS
from tests.test_gpu_pose import RAY_HI, RAY_LO, _device_bytes
from tests.test_gpu_refit import BOUNCES, HBM_KERNELS, SPP, _bits, _close, _ctx, _rays, _strict_bars

pytestmark = pytest.mark.gpu
NT = 706
UNITS = ("pose", "skin", "morph")


@pytest.fixture(scope="module")
def capi(built):
    from toyraygun_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def units(built):
    """The four modules, loaded: refit, and pose / skin / morph by name."""
    from toyraygun_amd import morph, pose, refit, skin
    for m in (refit, pose, skin, morph):
        m.load()
    return refit, {"pose": pose, "skin": skin, "morph": morph}


@pytest.fixture(scope="module")
def scene():
    """Scene A indexed and per corner, each with its targets and its skin binding; shared and left unchanged."""
    return {form: (b, MS.targets(b), SS.scene_a_binding(b)) for form, b in (("indexed", RS.scene_a_indexed(0)), ("per-corner", RS.scene_a(0)))}


def _bind(mods, c, unit, b, t, binding):
    if unit == "pose":
        mods[unit].bind(c, b["positions"], b["normals"], b["indices"], PS.scene_a_first())
    elif unit == "skin":
        mods[unit].bind(c, b["positions"], b["normals"], b["indices"], binding[0], binding[1], SS.N_BONES)
    else:
        mods[unit].bind(c, b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3], bone_ids=binding[0], bone_weights=binding[1], n_bones=SS.N_BONES)


def _inputs(unit, seed):
    """What apply of `unit` takes, a function of the seed (1, 2, 3): the inputs of the units' own tests."""
    if unit == "pose":
        return (PS.scene_a_xforms(seed),)
    if unit == "skin":
        return (SS.scene_a_bones(seed),)
    return (MS.weights("abc"[seed - 1]), SS.scene_a_bones(seed))


def _reference(mods, unit, b, t, binding, args):
    if unit == "pose":
        return mods[unit].pose_reference(b["positions"], b["normals"], b["indices"], PS.scene_a_first(), args[0])
    if unit == "skin":
        return mods[unit].skin_reference(b["positions"], b["normals"], b["indices"], binding[0], binding[1], args[0])
    return mods[unit].morph_reference(b["positions"], b["normals"], b["indices"], t[0], t[1], t[2], t[3], args[0], bone_ids=binding[0], bone_weights=binding[1], bones=args[1])


def _same(got, want):
    return np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _check_every_unit(mods, c, cur, prev, seen, what):
    """read of every unit is its expected current pose; its prev_pos / prev_nrm hold its own previous pose; no two units share a copy."""
    c.sync()
    now = []
    for u in UNITS:
        assert _same(mods[u].read(c), cur[u]), (what, u)
        p = mods[u].buffers(c)
        nv = cur[u][0].shape[0]
        assert np.array_equal(_device_bytes(p["prev_pos"], nv * 12), prev[u][0].view(np.uint8).reshape(-1)), (what, u)
        assert np.array_equal(_device_bytes(p["prev_nrm"], NT * 36), prev[u][1].view(np.uint8).reshape(-1)), (what, u)
        now += [p["pos"], p["prev_pos"], p["nrm"], p["prev_nrm"]]
        seen[u] |= {p["pos"], p["prev_pos"]}
    assert len(set(now)) == 12, what
    assert sum(len(seen[u]) for u in UNITS) == len(seen["pose"] | seen["skin"] | seen["morph"]), what


def _strict_state(capi, c, rays):
    c.set_option(capi.OPT_STRICT, 1)
    c.render(0, SPP, BOUNCES)
    img, tr = c.read_accum(), c.trace(rays)
    c.set_option(capi.OPT_STRICT, 0)
    return img, tr


def test_three_bindings_on_one_context_keep_to_themselves(capi, units, O, scene):
    """Pose, skin and morph (bones and normal deltas) bound together and applied interleaved: after EVERY apply the unit applied reads back its
    reference bit for bit and the other two what they held; each unit's previous-pose buffers hold its own previous pose; the nine position
    copies are nine allocations.  The loaded scene is the last apply's (strict frame and traces against the oracle).  An apply refused on the host
    (-22) changes none of it.  skin.release frees the skin unit alone; refit.release then unbinds all three, and the context still renders."""
    refit, mods = units
    b, t, binding = scene["indexed"]
    rest = (b["positions"], b["normals"])
    rays = _rays(O, 311, RAY_LO, RAY_HI)
    c = _ctx(capi, O, b, 0)
    try:
        for u in UNITS:
            _bind(mods, c, u, b, t, binding)
        cur, prev, seen = {u: rest for u in UNITS}, {u: rest for u in UNITS}, {u: set() for u in UNITS}
        _check_every_unit(mods, c, cur, prev, seen, "bound")
        args = None
        for step, (u, seed) in enumerate((("pose", 1), ("skin", 1), ("morph", 1), ("skin", 2), ("pose", 2), ("morph", 2))):
            args = _inputs(u, seed)
            mods[u].apply(c, *args)
            prev[u], cur[u] = cur[u], _reference(mods, u, b, t, binding, args)
            _check_every_unit(mods, c, cur, prev, seen, "apply %d: %s" % (step, u))
        assert all(len(seen[u]) == 3 for u in UNITS)                             # bound, applied twice: every unit has shown its three copies
        assert refit.refit_last(c)["path"] == refit.DEVICE
        moved = RS.unindexed(SS.posed_buffers(b, *cur["morph"]))
        _strict_bars(capi, O, c, RS.oracle_scene(O, moved), rays, "the last apply's geometry", kernels=HBM_KERNELS[:1])

        # a refused apply of one unit: every unit's current and previous pose, the frame and the trace stay
        before = _strict_state(capi, c, rays)
        nan = SS.scene_a_bones(3)
        nan[20, 7] = np.nan
        with pytest.raises(capi.TrgError) as e:
            mods["skin"].apply(c, nan)
        assert e.value.code == -22 and "bone 20" in str(e.value)
        _check_every_unit(mods, c, cur, prev, seen, "after the refusal")
        after = _strict_state(capi, c, rays)
        assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1].view(np.uint8), before[1].view(np.uint8))

        # release: one unit, then all
        mods["skin"].release(c)
        with pytest.raises(capi.TrgError) as e:
            mods["skin"].buffers(c)
        assert "bind" in str(e.value)
        for u in ("pose", "morph"):
            args = _inputs(u, 3)
            mods[u].apply(c, *args)
            assert _same(mods[u].read(c), _reference(mods, u, b, t, binding, args)), u
        before = _strict_state(capi, c, rays)
        refit.release(c)
        for u in UNITS:
            with pytest.raises(capi.TrgError) as e:
                mods[u].buffers(c)
            assert e.value.code == -22 and "bind" in str(e.value), u
        after = _strict_state(capi, c, rays)
        assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(after[1].view(np.uint8), before[1].view(np.uint8))
    finally:
        for u in UNITS:
            mods[u].release(c)
        _close(c, refit)


@pytest.mark.parametrize("unit", UNITS)
def test_a_rebind_at_another_size_leaves_the_other_units_alone(capi, units, scene, O, unit):
    """One unit bound again with the per-corner form of scene A (2,118 vertices where 424 were bound: its buffers grow): its read has the new
    shape and equals its reference; the other two keep their poses, their previous poses and their addresses."""
    refit, mods = units
    b, t, binding = scene["indexed"]
    b2, t2, binding2 = scene["per-corner"]
    others = [u for u in UNITS if u != unit]
    c = _ctx(capi, O, b, 0)
    try:
        cur = {}
        for u in UNITS:
            _bind(mods, c, u, b, t, binding)
            mods[u].apply(c, *_inputs(u, 1))
            cur[u] = _reference(mods, u, b, t, binding, _inputs(u, 1))
        c.sync()
        held = {u: mods[u].buffers(c) for u in others}
        _bind(mods, c, unit, b2, t2, binding2)
        pos, nrm = mods[unit].read(c)
        assert pos.shape == (3 * NT, 3) and _same((pos, nrm), (b2["positions"], b2["normals"]))              # bound: the rest pose
        args = _inputs(unit, 2)
        mods[unit].apply(c, *args)
        assert _same(mods[unit].read(c), _reference(mods, unit, b2, t2, binding2, args))
        c.sync()
        for u in others:
            assert mods[u].buffers(c) == held[u] and _same(mods[u].read(c), cur[u]), u
            assert np.array_equal(_device_bytes(held[u]["prev_pos"], b["positions"].shape[0] * 12), b["positions"].view(np.uint8).reshape(-1)), u
    finally:
        for u in UNITS:
            mods[u].release(c)
        _close(c, refit)
