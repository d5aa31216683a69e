"""The scene of the per_class fixtures (tests/golden/perclass_{deepoc,hybrid}_*.npz), shared by the
golden maker and the tests so that both regenerate the same frames from the fixture's arguments."""
import ast

import numpy as np

NR_CLASSES = 3
# identity k has class CLASSES[k % 12]: classes 0 and 1 are populated, class 2 never is, and two
# identities in 24 carry class 4 >= NR_CLASSES, whose rows the class split drops
CLASSES = (0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 4)


def perclass_frames(scene, n_frames, blank_class, blank_frames, start=0):
    """(frame number, dets, embs) of `scene` with the rows of `blank_class` taken out in
    `blank_frames`: there the class has live tracks and no detections.  Frames before `start`
    are not yielded (a sequence that starts late)."""
    for t in range(1, n_frames + 1):
        d, e, _ = scene.frame(t)
        if t in blank_frames:
            keep = d[:, 5] != blank_class
            d, e = d[keep], e[keep]
        if t > start:
            yield t, d, e


def fixture_frames(fx, seed=None, start=0):
    """The frames a fixture was captured on (seed: the same scene at another seed)."""
    from boxmot_amd.synth import SyntheticScene

    skw = ast.literal_eval(str(fx["scene"]))
    if seed is not None:
        skw["seed"] = seed
    blank = [int(t) for t in np.asarray(fx["blank_frames"]).reshape(-1)]
    return list(perclass_frames(SyntheticScene(**skw), int(fx["n_frames"]),
                                int(fx["blank_class"]), blank, start))
