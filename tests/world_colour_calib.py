"""CPU calibration of colour through the voxel store: the stream of tests/shift_calib.py (its volume, its
follow parameters, the ten frames of the calibration room) with the colour function of tests/colour_world.py, fused on
the restatements with the window following the camera, once through a colour store and once through a plain store.  The
frames are fused at their true poses, as the colour calibration of tests/test_colour_host.py fuses them, so the figures
speak of the store and not of the tracker; the window moves as shift_ref.follow says for those poses.  Afterwards the
colour at every surface point of the whole map (world_surface_ref.world_surface, store plus window) is compared with the
colour function at that point, per channel, in levels of 255.

    python tests/world_colour_calib.py [seed ...]
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camera_ref as E  # noqa: E402
import colour_ref as CR  # noqa: E402
import colour_world as CW  # noqa: E402
import reload_colour_ref as RC  # noqa: E402
import reload_ref as W  # noqa: E402
import shift_calib as SC  # noqa: E402
import shift_ref as H  # noqa: E402
import volume_ref as V  # noqa: E402
import world_colour_ref as WC  # noqa: E402
import world_surface_ref as WS  # noqa: E402


def volume():
    v = SC.VOLUME
    return CR.Volume(v["nx"], v["ny"], v["nz"], v["voxel"], v["origin"], mu=v["mu"], max_weight=v["max_weight"])


def run(synth, seed):
    """-> dict(colour=..., plain=...), each dict(points, share, median, p95, shifts, stored, reloaded): the whole map's
    surface points, the share of them with a colour and the error of those against the colour function"""
    world = E.make_world(synth, seed)
    rgb = CW.world_colours(world, seed)
    vols = dict(colour=volume(), plain=volume())
    stores = dict(colour=({}, {}), plain=({}, {}))
    counts = dict(shifts=0, stored=0, reloaded=0)
    for T in E.trajectory(synth, seed):
        depth, img, ok = CW.render(synth, world, rgb, T, **V.SMALL)
        z, rgba, T32 = V.z_image(depth, V.SMALL_CAM), CR.pack(img, ok), T.astype(np.float32)
        for vol in vols.values():
            vol.integrate_colour(z, rgba, V.SMALL_CAM, T32)
        s = H.follow(vols["colour"], T32, **SC.FOLLOW)
        if any(s):
            store, cstore = stores["colour"]
            vols["colour"], stored, reloaded = RC.shift_world(vols["colour"], store, cstore, s)
            counts = dict(shifts=counts["shifts"] + 1, stored=counts["stored"] + stored, reloaded=counts["reloaded"] + reloaded)
            # a plain store: the words go through it, the colours move as under the plain shift and what left is lost
            store = stores["plain"][0]
            colours = CR.shifted(vols["plain"], s).c
            vols["plain"], _, _ = W.shift_world(vols["plain"], store, s)
            vols["plain"].c = colours
    out = {}
    params = (SC.VOLUME["voxel"], np.asarray(SC.VOLUME["origin"], np.float32))
    for name in ("colour", "plain"):
        store, cstore = stores[name]
        if name == "plain":
            cstore = dict.fromkeys(store, 0)
        vol = vols[name]
        xyz, _, _, _ = WS.world_surface(store, params, vol)
        got, valid = WC.colours(store, cstore, params, xyz, vol)
        want = CW.colour(xyz.astype(np.float64), seed)
        err = np.abs(got[valid].astype(np.float64) - want[valid])
        out[name] = dict(points=len(xyz), share=float(valid.mean()), median=float(np.median(err)), p95=float(np.percentile(err, 95)),
                         store=len(store), **counts)
        assert not got[~valid].any()
    assert W.words_of(vols["colour"]).tobytes() == W.words_of(vols["plain"]).tobytes() and stores["colour"][0] == stores["plain"][0]
    return out


def main():
    synth = importlib.import_module("objective-slam_amd").synth
    for seed in [int(x) for x in sys.argv[1:]] or [0, 1, 2]:
        for name, r in run(synth, seed).items():
            print("seed %d, %s store: %d surface points of the whole map, %.4f with a colour, error median %.2f, 95th percentile "
                  "%.2f levels; %d shifts, %d stored, %d reloaded, %d in the store" % (
                      seed, name, r["points"], r["share"], r["median"], r["p95"], r["shifts"], r["stored"], r["reloaded"], r["store"]))


if __name__ == "__main__":
    main()
