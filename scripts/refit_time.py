"""Update time and render time of a refitted scene against a reloaded one (include/trg_refit.h).

    python scripts/refit_time.py [--n 44] [--reps 5] [--w 1024 --h 768 --spp 4] [--legs refit,pose,skin,morph,rig] [--parent-so FILE] [--out FILE]

The Cornell box + n^3 cubes (n = 44: 1,022,244 triangles, n = 96: 10,616,868).  In ONE process, alternating, medians over `reps`:

  update   trg_load_scene with the host builder, with TRG_OPT_GPU_BUILD=1, and trg_refit_scene of a tree of either builder -- with the positions
           as they are (identity) and with every cube moved by its own small translation -- each followed by a wait for the stream;
  render   ms per step of the tree as loaded, after an identity refit, after the small motion (with trg_refit_info's area ratio beside it) and
           of a fresh load of the moved geometry, for both builders.

The pose leg (include/trg_pose.h; device builder): objects = the Cornell box + one per cube, every cube moved by the same small translation, now as a
matrix.  Alternating, medians over `reps`, each call followed by a wait for the stream: trg_pose_apply; trg_refit_scene_device from torch tensors
of the same posed geometry; trg_refit_scene from host arrays of it; and -- with --parent-so, the library of the parent commit built into a side
directory -- that library's trg_refit_scene in a context of its own.  Beside them the render time per step after a pose, and what the posing costs
on top of the refit it feeds (trg_pose_apply minus trg_refit_scene_device: the 48-byte-per-object upload and the kernel).  The pose kernel's OWN time
is not a host-side figure: run this leg once more under a kernel trace,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/refit_time.py --legs pose
and read rf_pose_kernel's row of the kernel statistics (without --output-format the run leaves a results database whose `kernels` view has one
row per launch with its duration in ns).

The skin leg (include/trg_skin.h; device builder): bones = the Cornell box's + one per cube; every vertex names FOUR DISTINCT bones (its own and
the next three), its weight 1 on its own -- the kernel's work does not depend on the weights' values --, every cube's bone the same small
translation.  Alternating, medians over `reps`, each call followed by a wait: trg_skin_apply; trg_refit_scene_device and trg_refit_scene of the same
skinned geometry; with --parent-so that library's trg_refit_scene.  rf_skin_kernel's own time: the same kernel-trace run, with --legs skin.

The morph leg (include/trg_morph.h; device builder): eight targets -- two dense (every cube shifted by its own vector; every cube stretched about
its own centre) and six that each shift a sixth of the cubes --, so every vertex holds three entries; two weight vectors with three active targets
each alternate, so that no apply is a no-op.  Without bones, and with the skin leg's four-distinct-bones binding behind the targets.  Alternating,
medians over `reps`, each call followed by a wait, both libraries straight through ctypes: trg_morph_apply; trg_skin_apply; trg_refit_scene of the
same morphed geometry; with --parent-so that library's trg_refit_scene -- what a caller with blend shapes pays today, before the CPU morph itself.
rf_morph_kernel's own time: the same kernel-trace run, with --legs morph.

The rig leg (include/trg_rig.h; device builder): the skin leg's binding, and a rig of one five-joint chain per five bones (n = 44: 17,037 chains,
85,185 joints), two keys per joint, one clock per chain, no inverse binds; two clock vectors alternate.  Alternating, medians over `reps`, each call
followed by a wait, both libraries straight through ctypes: trg_rig_skin_apply; trg_rig_skin_apply_device from a torch tensor of the same bones;
this library's trg_skin_apply and -- with --parent-so -- the parent's, given those bones PRECOMPUTED on the host: what a caller pays today, not
counting the CPU evaluation of the skeleton.  rig_skin_apply_not_slower_than_parent_skin_apply compares the medians.  rf_rig_level_kernel's own
time: the same kernel-trace run, with --legs rig.

Every apply and every trg_refit_scene is called straight through ctypes, as the parent's are (the wrappers' argument checks cost about 10 us, the
size of the differences looked for; the skin leg times refit.py's wrapper beside them).  With --parent-so every leg
also binds the same data on the parent library, when it exports the leg's symbols, and times ITS trg_{pose,skin,morph}_apply in the same alternation:
parent_<call>, and <call>_within_parent_spread -- this build's median lies between the smallest and the largest of the parent's samples.

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from toyraygun_amd import capi, host, morph, pose, refit, rig, skin  # noqa: E402


def parent_context(path, w, h, pos, nrm, col, idx, mat):
    """A context of ANOTHER build of the library (ctypes keeps the two apart), device-built scene loaded: (library, handle)."""
    import ctypes as C
    L = C.CDLL(path)
    for name, res, args in capi._SYMBOLS + refit._SYMBOLS + pose._SYMBOLS + skin._SYMBOLS + morph._SYMBOLS:
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    h_ctx = C.c_void_p()
    assert L.trg_create(C.byref(h_ctx), 0, w, h) == 0
    assert L.trg_set_option(h_ctx, capi.OPT_GPU_BUILD, 1) == 0
    assert L.trg_load_scene(h_ctx, pos.ctypes.data, nrm.ctypes.data, col.ctypes.data, idx.ctypes.data, mat.ctypes.data, pos.shape[0], mat.shape[0]) == 0
    return L, h_ctx


def raw(L, h, name, *args):
    """A C call of either library straight through ctypes (arrays by their address, None as it is), then the wait for its stream."""
    rc = getattr(L, name)(h, *[x.ctypes.data if isinstance(x, np.ndarray) else x for x in args])
    assert rc == 0, (name, L.trg_last_error(h))
    L.trg_sync(h)


def cube_bones(n_verts, n_cubes, d):
    """One bone for the Cornell box and one per cube: (ids, weights, bones at rest, bones moved, n_bones).  Every vertex names FOUR DISTINCT bones
    (its own and the next three), its weight 1 on its own; every cube's moved bone is its translation d.  (The pose leg's objects are these bones.)"""
    n_bones = n_cubes + 1
    own = np.concatenate([np.zeros(108, np.int64), 1 + np.repeat(np.arange(n_cubes), 36)])
    ids = ((own[:, None] + np.arange(4)[None, :]) % n_bones).astype(np.uint32)
    wts = np.zeros((n_verts, 4), np.float32)
    wts[:, 0] = 1.0
    x0 = np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (n_bones, 1))
    x1 = x0.copy()
    x1[1:, [3, 7, 11]] = d
    return ids, wts, x0, x1, n_bones


def alternate(calls, reps, timed):
    """Every call once (scratch is allocated once, and every call is accepted), then alternating `reps` times: {name: [ms]}.  A call takes the
    round's number: calls that alternate between two inputs are never a no-op."""
    for f in calls.values():
        f(0)
    t = {k: [] for k in calls}
    for k in range(reps):
        for name, f in calls.items():
            t[name].append(timed(lambda: f(k)))
    return t


def medians(t, key=lambda k: k):
    """{<key>_ms: the median, <key>_ms_all: every sample} of alternate()'s samples."""
    r = {key(k) + "_ms": statistics.median(v) for k, v in t.items()}
    r.update({key(k) + "_ms_all": [round(x, 3) for x in v] for k, v in t.items()})
    return r


def within_spread(t, ours, parents):
    return bool(min(t[parents]) <= statistics.median(t[ours]) <= max(t[parents]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=44)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--h", type=int, default=768)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--legs", default="refit,pose")
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    b = host.Scene.cornell_lattice(a.n).buffers()
    pos0, nrm, col, idx, mat = b["positions"], b["normals"], b["colors"], b["indices"], b["material_ids"]
    nt = mat.shape[0]
    # every cube of the lattice (36 vertices each, behind the Cornell box's 108) moved by its own translation, a multiple of 2^-11 of at most 2^-9
    # per axis: the sums are exact or lose one bit, so a cube stays the parallelepiped it was to the builders' tolerances
    rng = np.random.default_rng(7)
    n_cubes = (pos0.shape[0] - 108) // 36
    d = (rng.integers(-4, 5, (n_cubes, 3)).astype(np.float32) * np.float32(2.0 ** -11))
    pos1 = pos0.copy()
    pos1[108:108 + 36 * n_cubes] += np.repeat(d, 36, axis=0)

    c = capi.Context(a.w, a.h)
    c.set_uniforms(host.uniforms(a.w, a.h)[0])
    c.set_pixel_offsets_seed()
    res = {"triangles": int(nt), "reps": a.reps, "image": [a.w, a.h, a.spp, a.bounces]}

    def timed(f):
        c.sync()
        t0 = time.perf_counter()
        f()
        c.sync()
        return (time.perf_counter() - t0) * 1e3

    def load(builder, pos):
        c.set_option(capi.OPT_GPU_BUILD, builder)
        c.load_scene(pos, nrm, col, idx, mat)

    def render_ms():
        c.render(0, a.spp, a.bounces)                                      # warm-up (scratch, caches)
        return statistics.median(timed(lambda: c.render(0, a.spp, a.bounces)) for _ in range(a.reps)) / a.spp

    try:
        for builder, name in ((0, "host"), (1, "device")) if "refit" in a.legs.split(",") else ():
            t = {"load": [], "refit_identity": [], "refit_moved": []}
            load(builder, pos0)
            refit.refit_scene(c, pos0, nrm, idx)                           # (the scratch is allocated once)
            for _ in range(a.reps):                                        # alternating: load, identity refit, moved refit
                t["load"].append(timed(lambda: load(builder, pos0)))
                t["refit_identity"].append(timed(lambda: refit.refit_scene(c, pos0, nrm, idx)))
                t["refit_moved"].append(timed(lambda: refit.refit_scene(c, pos1, nrm, idx)))
            info_moved = refit.refit_last(c)
            r = {k + "_ms": statistics.median(v) for k, v in t.items()}
            r.update({k + "_ms_all": [round(x, 3) for x in v] for k, v in t.items()})
            load(builder, pos0)
            r["build_ms_of_load"] = c.stats().last_build_ms              # the builder's own share of a load
            # render time: as loaded, identity refit, moved refit, fresh load of the moved geometry
            load(builder, pos0)
            r["render_loaded_ms"] = render_ms()
            refit.refit_scene(c, pos0, nrm, idx)
            r["identity_area_ratio"] = refit.refit_last(c)["area_ratio"]
            r["render_refit_identity_ms"] = render_ms()
            refit.refit_scene(c, pos1, nrm, idx)
            i = refit.refit_last(c)
            r["moved_area_ratio"], r["moved_area_ratio_box"], r["passes"], r["path"] = i["area_ratio"], i["area_ratio_box"], i["passes"], i["path_name"]
            r["n_quads"], r["n_boxes"] = i["n_quads"], i["n_boxes"]
            r["render_refit_moved_ms"] = render_ms()
            load(builder, pos1)
            r["render_fresh_moved_ms"] = render_ms()
            r["refit_last_ms_moved"] = info_moved["ms"]
            res[name] = r
        if "device" in res:
            res["refit_beats_device_rebuild"] = bool(res["device"]["refit_moved_ms"] < res["device"]["load_ms"] and res["host"]["refit_moved_ms"] < res["device"]["load_ms"])
        RL, PoL, SL, ML = refit.load(), pose.load(), skin.load(), morph.load()
        nv = pos0.shape[0]
        ids, wts, x0, x1, n_bones = cube_bones(nv, n_cubes, d)

        def refit_calls(parent, moved, tensors=None):
            # trg_refit_scene of this library and of the parent's are called the same way, straight through ctypes (the size of the difference looked
            # for is the wrapper's 10 us); trg_refit_scene_device from torch tensors of the same geometry
            calls = {"refit_scene": lambda k: raw(RL, c.h_ctx, "trg_refit_scene", moved, nrm, idx, nv, nt)}
            if tensors:
                calls["refit_scene_device"] = lambda k: pose.refit_scene_device(c, *tensors)
            if parent:
                calls["parent_refit_scene"] = lambda k: raw(parent[0], parent[1], "trg_refit_scene", moved, nrm, idx, nv, nt)
            return calls

        def device_tensors():
            import torch
            t = torch.from_numpy(pos1).cuda(), torch.from_numpy(nrm).cuda(), torch.from_numpy(idx.view(np.int32)).cuda()
            torch.cuda.synchronize()
            return t

        if "pose" in a.legs.split(","):
            first = np.concatenate([[0], 36 + 12 * np.arange(n_cubes + 1)]).astype(np.uint32)
            load(1, pos0)
            pose.bind(c, pos0, nrm, idx, first)
            pose.apply(c, x1)
            got, _ = pose.read(c, nv, nt)
            assert (got == pos1).all()                                     # the same posed geometry as the host arrays of the refit leg
            parent = parent_context(a.parent_so, a.w, a.h, pos0, nrm, col, idx, mat) if a.parent_so else None
            calls = {"pose_apply": lambda k: raw(PoL, c.h_ctx, "trg_pose_apply", (x1, x0)[k % 2])}
            calls.update(refit_calls(parent, pos1, device_tensors()))
            if parent and hasattr(parent[0], "trg_pose_apply"):
                raw(parent[0], parent[1], "trg_pose_bind", pos0, nrm, idx, nv, nt, first, n_bones)
                calls["parent_pose_apply"] = lambda k: raw(parent[0], parent[1], "trg_pose_apply", (x1, x0)[k % 2])
            t = alternate(calls, a.reps, timed)
            r = medians(t)
            r["objects"] = int(n_bones)
            r["upload_bytes"] = {"pose_apply": int(48 * n_bones), "refit_scene": int(pos1.nbytes + idx.nbytes + nrm.nbytes)}
            r["posing_on_top_of_the_refit_ms"] = r["pose_apply_ms"] - r["refit_scene_device_ms"]    # upload of the matrices + rf_pose_kernel
            pose.apply(c, x1)
            r["render_after_pose_ms"] = render_ms()
            r["pose_not_slower_than_refit_scene"] = bool(r["pose_apply_ms"] <= r["refit_scene_ms"])
            if "parent_pose_apply" in t:
                r["pose_apply_within_parent_spread"] = within_spread(t, "pose_apply", "parent_pose_apply")
            res["pose"] = r
            if parent:
                parent[0].trg_destroy(parent[1])
        if "skin" in a.legs.split(","):
            load(1, pos0)
            skin.bind(c, pos0, nrm, idx, ids, wts, n_bones)
            skin.apply(c, x1)
            got, _ = skin.read(c)
            assert (got == pos1).all()                                     # the same geometry as the host arrays of the refit leg
            parent = parent_context(a.parent_so, a.w, a.h, pos0, nrm, col, idx, mat) if a.parent_so else None
            calls = {"skin_apply": lambda k: raw(SL, c.h_ctx, "trg_skin_apply", (x1, x0)[k % 2])}
            calls.update(refit_calls(parent, pos1, device_tensors()))
            calls["refit_scene_through_refit_py"] = lambda k: refit.refit_scene(c, pos1, nrm, idx)
            if parent and hasattr(parent[0], "trg_skin_apply"):
                raw(parent[0], parent[1], "trg_skin_bind", pos0, nrm, idx, nv, nt, ids, wts, n_bones)
                calls["parent_skin_apply"] = lambda k: raw(parent[0], parent[1], "trg_skin_apply", (x1, x0)[k % 2])
            t = alternate(calls, a.reps, timed)
            r = medians(t)
            r["bones"] = int(n_bones)
            r["vertices"] = int(nv)
            r["upload_bytes"] = {"skin_apply": int(48 * n_bones), "refit_scene": int(pos1.nbytes + idx.nbytes + nrm.nbytes)}
            r["skinning_on_top_of_the_refit_ms"] = r["skin_apply_ms"] - r["refit_scene_device_ms"]  # upload of the bones + rf_skin_kernel
            # what rf_skin_kernel streams: 16 + 16 + 12 + 12 per vertex, 4 + 16 + 16 + 12 + 12 per corner (the bones come from cache)
            r["kernel_streamed_bytes"] = int(56 * nv + 60 * 3 * nt)
            skin.apply(c, x1)
            r["render_after_skin_ms"] = render_ms()
            if parent:
                r["skin_not_slower_than_parent_refit_scene"] = bool(r["skin_apply_ms"] <= r["parent_refit_scene_ms"])
                r["refit_scene_within_parent_spread"] = within_spread(t, "refit_scene", "parent_refit_scene")
                if "parent_skin_apply" in t:
                    r["skin_apply_within_parent_spread"] = within_spread(t, "skin_apply", "parent_skin_apply")
                parent[0].trg_destroy(parent[1])
            skin.release(c)
            res["skin"] = r
        if "morph" in a.legs.split(","):
            cube = np.concatenate([np.full(108, -1, np.int64), np.repeat(np.arange(n_cubes), 36)])      # vertex -> cube (-1: the Cornell box)
            centre = pos0[108:108 + 36 * n_cubes].astype(np.float64).reshape(n_cubes, 36, 3).mean(1)
            shift = np.concatenate([np.zeros((108, 3), np.float32), np.repeat(d, 36, axis=0)])
            stretch = np.zeros((nv, 3), np.float32)
            stretch[108:] = (2.0 ** -5 * (pos0[108:].astype(np.float64) - np.repeat(centre, 36, axis=0))).astype(np.float32)
            d6 = (rng.integers(-4, 5, (n_cubes, 3)).astype(np.float32) * np.float32(2.0 ** -11))
            sixth = np.where(cube < 0, 0, cube % 6)
            ev = [np.arange(nv), np.arange(nv)] + [np.flatnonzero(sixth == j) for j in range(6)]
            dp = [shift, stretch] + [np.where(cube[v, None] < 0, np.float32(0), d6[np.maximum(cube[v], 0)]).astype(np.float32) for v in ev[2:]]
            first = np.concatenate([[0], np.cumsum([v.shape[0] for v in ev])]).astype(np.uint32)
            ev, dp = np.concatenate(ev).astype(np.uint32), np.ascontiguousarray(np.concatenate(dp))
            assert (np.bincount(ev, minlength=nv) == 3).all()              # every vertex holds three entries
            wA, wB = np.array([1, 0.5, 1, 0, 0, 0, 0, 0], np.float32), np.array([0.5, 1, 0, 0, 1, 0, 0, 1], np.float32)
            load(1, pos0)
            parent = parent_context(a.parent_so, a.w, a.h, pos0, nrm, col, idx, mat) if a.parent_so else None
            parent_morphs = parent and hasattr(parent[0], "trg_morph_apply")
            skin.bind(c, pos0, nrm, idx, ids, wts, n_bones)
            r = {"vertices": int(nv), "targets": 8, "entries": int(ev.shape[0]), "bones": int(n_bones)}
            for with_bones in (False, True):
                tag = "morph_apply_bones" if with_bones else "morph_apply"
                morph.bind(c, pos0, nrm, idx, first, ev, dp, None, **(dict(bone_ids=ids, bone_weights=wts, n_bones=n_bones) if with_bones else {}))
                morph.apply(c, wA, x1 if with_bones else None)
                got, _ = morph.read(c)
                ref, _ = morph.morph_reference(pos0, None, idx, first, ev, dp, None, wA, **(dict(bone_ids=ids, bone_weights=wts, bones=x1) if with_bones else {}))
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
                posA = np.ascontiguousarray(got)                           # the morphed geometry a caller would have made on the CPU
                bones = (x1, x0) if with_bones else (None, None)
                calls = {tag: lambda k: raw(ML, c.h_ctx, "trg_morph_apply", (wA, wB)[k % 2], bones[k % 2]),
                         "skin_apply": lambda k: raw(SL, c.h_ctx, "trg_skin_apply", (x1, x0)[k % 2])}
                calls.update(refit_calls(parent, posA))
                if parent_morphs:
                    raw(parent[0], parent[1], "trg_morph_bind", pos0, nrm, idx, nv, nt, 8, first, int(ev.shape[0]), ev, dp, None,
                        *((ids, wts, n_bones) if with_bones else (None, None, 0)))
                    calls["parent_" + tag] = lambda k: raw(parent[0], parent[1], "trg_morph_apply", (wA, wB)[k % 2], bones[k % 2])
                t = alternate(calls, a.reps, timed)
                r.update(medians(t, lambda k: k if k.endswith(tag) else k + ("_beside_bones" if with_bones else "")))
                if parent:
                    r[tag + "_not_slower_than_parent_refit_scene"] = bool(statistics.median(t[tag]) <= statistics.median(t["parent_refit_scene"]))
                if parent_morphs:
                    r[tag + "_within_parent_spread"] = within_spread(t, tag, "parent_" + tag)
            r["upload_bytes"] = {"morph_apply": 4 * 8, "morph_apply_bones": int(4 * 8 + 48 * n_bones), "refit_scene": int(pos0.nbytes + idx.nbytes + nrm.nbytes)}
            # what rf_morph_kernel streams.  Without bones (no normal deltas: the corner range is not launched): 12 in, 12 out, one range word and
            # three 16-byte records per vertex.  With bones: 16 + 16 more per vertex, and 4 + 16 + 16 + 12 + 12 per corner (the bones and the
            # weights come from cache)
            r["kernel_streamed_bytes"] = {"morph_apply": int((12 + 12 + 4 + 48) * nv), "morph_apply_bones": int((12 + 12 + 4 + 48 + 32) * nv + 60 * 3 * nt),
                                          "skin_apply": int(56 * nv + 60 * 3 * nt)}
            r["render_after_morph_ms"] = render_ms()
            if parent:
                parent[0].trg_destroy(parent[1])
            morph.release(c)
            skin.release(c)
            res["morph"] = r
        if "rig" in a.legs.split(","):
            import torch
            GL = rig.load()
            assert n_bones % 5 == 0
            n_chains = n_bones // 5
            j = np.arange(n_bones)
            par = np.where(j % 5 == 0, rig.NO_PARENT, j - 1).astype(np.uint32)
            keys = np.zeros((2 * n_bones, 12), np.float32)
            keys[:, 7] = 1.0                                                # no rotation
            keys[:, 8:11] = 1.0
            keys[1::2, 0] = 1.0                                             # key 0 at time 0: rest; key 1 at time 1: a small translation per joint
            keys[1::2, 1:4] = rng.integers(-4, 5, (n_bones, 3)).astype(np.float32) * np.float32(2.0 ** -11)
            kfirst = (2 * np.arange(n_bones + 1)).astype(np.uint32)
            clock_of = (j // 5).astype(np.uint32)
            clocks = [np.full(n_chains, 1.0, np.float32), np.linspace(0.25, 0.75, n_chains).astype(np.float32)]
            bones = [rig.rig_reference(par, kfirst, keys, clock_of, t)[0] for t in clocks]     # the caller's CPU evaluation, outside every timing
            load(1, pos0)
            skin.bind(c, pos0, nrm, idx, ids, wts, n_bones)
            rig.bind(c, par, kfirst, keys, clock_of, n_chains)
            rig.skin_apply(c, clocks[0])
            got = rig.read(c)[0], skin.read(c)[0]
            assert np.array_equal(got[0].view(np.uint32), bones[0].view(np.uint32))
            skin.apply(c, bones[0])
            assert np.array_equal(skin.read(c)[0].view(np.uint32), got[1].view(np.uint32))     # the same skinned geometry either way
            tensors = [torch.from_numpy(x).cuda() for x in bones]
            torch.cuda.synchronize()
            parent = parent_context(a.parent_so, a.w, a.h, pos0, nrm, col, idx, mat) if a.parent_so else None
            calls = {"rig_skin_apply": lambda k: raw(GL, c.h_ctx, "trg_rig_skin_apply", clocks[k % 2]),
                     "rig_skin_apply_device": lambda k: raw(GL, c.h_ctx, "trg_rig_skin_apply_device", tensors[k % 2].data_ptr()),
                     "skin_apply": lambda k: raw(SL, c.h_ctx, "trg_skin_apply", bones[k % 2])}
            if parent:
                raw(parent[0], parent[1], "trg_skin_bind", pos0, nrm, idx, nv, nt, ids, wts, n_bones)
                calls["parent_skin_apply"] = lambda k: raw(parent[0], parent[1], "trg_skin_apply", bones[k % 2])
            t = alternate(calls, a.reps, timed)
            r = medians(t)
            r.update({"joints": int(n_bones), "chains": int(n_chains), "levels": 5, "keys": int(keys.shape[0]), "vertices": int(nv)})
            r["upload_bytes"] = {"rig_skin_apply": int(4 * n_chains), "rig_skin_apply_device": 0, "skin_apply": int(48 * n_bones)}
            # what rf_rig_level_kernel moves per joint: order, clock id, two key-range words, two 48-byte keys, world and bone rows out -- and from
            # level 1 on the parent's id and its world rows (the clocks come from cache; there are no inverse binds here)
            r["kernel_moved_bytes"] = int((4 + 4 + 8 + 96 + 96) * n_bones + (4 + 48) * (n_bones - n_chains))
            r["evaluation_on_top_of_the_device_form_ms"] = r["rig_skin_apply_ms"] - r["rig_skin_apply_device_ms"]
            if parent:
                r["rig_skin_apply_not_slower_than_parent_skin_apply"] = bool(r["rig_skin_apply_ms"] <= r["parent_skin_apply_ms"])
                r["skin_apply_within_parent_spread"] = within_spread(t, "skin_apply", "parent_skin_apply")
                parent[0].trg_destroy(parent[1])
            rig.release(c)
            skin.release(c)
            res["rig"] = r
    finally:
        refit.release(c)
        c.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
