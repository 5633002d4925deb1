"""The roidbs shared by tests/golden/make_golden_data_layer.py and tests/test_data_layer_cpu.py (the fixture stores
results only): 5 supervised and 7 weak entries on the five sample shapes, some flipped."""
import numpy as np

from image_inputs import SHAPES, synth_plane

IMS_PER_BATCH, WS_IMS_PER_BATCH, SEED, FORWARDS = 2, 3, 3, 6


def make_roidbs():
    """-> (roidb_s, roidb_ws, planes): entries {'image': key, 'flipped', 'boxes' u16, 'gt_classes' i32, 'birads_diag'};
    planes[key] = the decoded plane."""
    rs = np.random.RandomState(77)
    planes, out = {}, []
    for tag, n in (("s", 5), ("w", 7)):
        db = []
        for i in range(n):
            h, w = SHAPES[(i + (tag == "w")) % len(SHAPES)]
            key = "%s%d" % (tag, i)
            planes[key] = synth_plane(500 + 10 * (tag == "w") + i, h, w)
            k = int(rs.randint(1, 4))
            x1, y1 = rs.randint(0, w // 2, size=k), rs.randint(0, h // 2, size=k)
            boxes = np.stack([x1, y1, x1 + rs.randint(8, w // 2, size=k), y1 + rs.randint(8, h // 2, size=k)],
                             axis=1).astype(np.uint16)
            db.append(dict(image=key, flipped=bool(i % 3 == 1), boxes=boxes,
                           gt_classes=rs.randint(0, 3, size=k).astype(np.int32), birads_diag=int(rs.randint(1, 3))))
        out.append(db)
    return out[0], out[1], planes
