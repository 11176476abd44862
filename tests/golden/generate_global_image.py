"""Generates tests/golden/global_image/global_image.npz: `Warehouse.get_global_image(layers, recompute=True)` of the UNMODIFIED reference
after every step of the golden traces next to this directory (same kwargs, seeds, actions, NEXT_STEP autoreset, pinned tie-break — see
generate_golden.py), for the layer lists in CASES.
Run in the build container:  python tests/golden/generate_global_image.py

The replay is checked against the stored trace (rewards, done) step by step, so the images belong to exactly those traces.  Per case,
with key = "<trace>/<layers joined by '-'>":
    <key>/image    uint8 [T][E][C][H][W]  the image after step t (every element of a global image is an integer in 0 .. 4); zeros where
                                          the call raised
    <key>/raised   uint8 [T][E]           1: the call raised IndexError — AGENT_DIRECTION / AGENT_LOAD are written at `[ag.x, ag.y]` of an
                                          (H, W) array (rware/warehouse.py:1003, :1008), which leaves it once x >= H or y >= W
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
import ref_runner as rr  # noqa: E402

ALL7 = [0, 1, 2, 3, 4, 5, 6]
# tiny-2ag is 11 x 10 (H > W): its agents reach y >= W, where the two transposed layers raise — they are recorded as lists of their own,
# so that the five other layers of those steps still have an image
CASES = [("img-square-all7-msg1", ALL7), ("layoutstr-3ag", ALL7), ("tiny-2ag", [0, 1, 2, 5, 6]), ("tiny-2ag", [3]), ("tiny-2ag", [4])]


def key_of(name, layers):
    return name + "/" + "-".join(str(l) for l in layers)


def images_of(name, layer_lists):
    wh = rr.load_reference()
    meta, z = gu.load_fixture(name)
    kw = dict(meta["kwargs"])
    kw["reward_type"] = wh.RewardType(kw["reward_type"])
    kw["observation_type"] = wh.ObservationType(int(kw.get("observation_type", 1)))
    if "image_observation_layers" in kw:
        kw["image_observation_layers"] = [wh.ImageLayer(int(l)) for l in kw["image_observation_layers"]]
    E, T, M = meta["E"], meta["T"], int(kw.get("msg_bits", 0))
    envs = [wh.Warehouse(**kw) for _ in range(E)]
    for e, env in enumerate(envs):
        env.reset(seed=meta["seed"] + e)
    H, W = envs[0].grid_size
    out = {tuple(ls): (np.zeros((T, E, len(ls), H, W), np.uint8), np.zeros((T, E), np.uint8)) for ls in layer_lists}
    for t in range(T):
        for e, env in enumerate(envs):
            if z["was_reset"][t][e]:
                env.reset()
            else:
                a = z["actions"][t][e]
                a = [[int(v) for v in row] for row in a] if M else [int(v) for v in a]
                _, r, d, _, _ = rr.ref_step(env, a)
                assert np.array_equal(np.asarray(r, np.float32), z["rewards"][t][e]) and int(bool(d)) == int(z["done"][t][e]), (name, t, e)
            for ls, (image, raised) in out.items():
                try:
                    img = env.get_global_image([wh.ImageLayer(l) for l in ls], recompute=True)
                except IndexError:
                    raised[t, e] = 1
                    continue
                assert img.dtype == np.float32 and img.shape == image.shape[2:] and np.array_equal(img, img.astype(np.uint8))
                image[t, e] = img.astype(np.uint8)
    return out


if __name__ == "__main__":
    out, summary = {}, {}
    for name in sorted({n for n, _ in CASES}):
        for ls, (image, raised) in images_of(name, [ls for n, ls in CASES if n == name]).items():
            k = key_of(name, ls)
            out[k + "/image"], out[k + "/raised"] = image, raised
            steps = raised.any(axis=1)
            summary[k] = {"shape": list(image.shape), "steps_raised": int(steps.sum()), "steps_clean": int((~steps).sum())}
            print(k, summary[k])
    os.makedirs(os.path.join(HERE, "global_image"), exist_ok=True)
    path = os.path.join(HERE, "global_image", "global_image.npz")
    np.savez_compressed(path, meta=json.dumps({
        "source": "semitable/robotic-warehouse (rware 2.0.0), unmodified, pinned tie-break",
        "gymnasium": "standin" if rr.using_standin_gymnasium() else "real", "cases": summary}), **out)
    print(os.path.getsize(path), "bytes")
