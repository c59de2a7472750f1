"""Shared by tools/gen_openpose_golden.py and the OpenPose tests: a torch restatement of the reference's bodypose_model forward
(openpose/model.py:111-124), pinned to the imported module by tests/test_openpose_model.py, and the planted stage-6 outputs.

The planted maps use only +, -, *, / and sqrt (correctly rounded in IEEE arithmetic), so every machine builds the same bits and the
golden needs to store only the reference's answer for them."""
import numpy as np

PLANT_HW = (160, 200)
# COCO-18 joints (x, y) in original pixels: a whole person, one without a neck (its face and arm subsets merge, found == 2) and a
# lone forearm (a two-part subset that is deleted)
PEOPLE = (
    {0: (50, 30), 1: (50, 48), 2: (36, 50), 3: (30, 72), 4: (28, 94), 5: (64, 50), 6: (70, 72), 7: (72, 94), 8: (42, 98),
     9: (40, 124), 10: (40, 148), 11: (58, 98), 12: (60, 124), 13: (60, 148), 14: (46, 26), 15: (54, 26), 16: (42, 30), 17: (58, 30)},
    {0: (140, 32), 2: (126, 54), 3: (120, 76), 4: (118, 98), 14: (136, 28), 15: (144, 28), 16: (131, 33), 17: (149, 33)},
    {6: (160, 120), 7: (176, 140)},
)


def planted_outputs(H=PLANT_HW[0], W=PLANT_HW[1]):
    """per scale float32 [hq, wq, 57]: a bump (1 - d^2 / 9)^2 of radius 3 cells at each joint in its heat channel, the limb's unit
    vector within 1 cell of each limb in its two PAF channels"""
    from bodyfitting_amd import openpose as O
    outs = []
    for s, (h, w, Hp, Wp) in zip(O.scales(H), O.scale_dims(H, W)):
        hq, wq = Hp // 8, Wp // 8
        o = np.zeros((hq, wq, O.N_OUT), np.float32)
        yy, xx = np.mgrid[0:hq, 0:wq].astype(np.float64)
        cell = lambda p: ((p[0] + 0.5) * s / 8 - 0.5, (p[1] + 0.5) * s / 8 - 0.5)
        for person in PEOPLE:
            for j, p in person.items():
                cx, cy = cell(p)
                d2 = (xx - cx) * (xx - cx) + (yy - cy) * (yy - cy)
                bump = np.where(d2 < 9.0, (1.0 - d2 / 9.0) * (1.0 - d2 / 9.0), 0.0)
                o[..., O.N_PAF + j] = np.maximum(o[..., O.N_PAF + j], bump)
            for k, (a, b) in enumerate(O.LIMB_SEQ):
                if a - 1 not in person or b - 1 not in person:
                    continue
                (ax, ay), (bx, by) = cell(person[a - 1]), cell(person[b - 1])
                L = np.sqrt((bx - ax) * (bx - ax) + (by - ay) * (by - ay))
                ux, uy = (bx - ax) / L, (by - ay) / L
                t = (xx - ax) * ux + (yy - ay) * uy
                d = np.abs((xx - ax) * uy - (yy - ay) * ux)
                band = (t >= -1) & (t <= L + 1) & (d <= 1.0)
                o[..., O.MAP_IDX[k][0] - 19][band] = ux
                o[..., O.MAP_IDX[k][1] - 19][band] = uy
        outs.append(o)
    return outs


def bodypose_forward(state, x, dtype):
    """bodypose_model.forward on x [1, 3, H, W] (numpy, NCHW) with the caffe-keyed state dict, in `dtype` (torch.float32 / float64) ->
    [H/8, W/8, 57] numpy (Mconv7_stage6_L1 0:38, Mconv7_stage6_L2 38:57).  Mconv7_stage6_L2 keeps its ReLU (model.py:29-32)."""
    import torch
    import torch.nn.functional as F
    from bodyfitting_amd import openpose as O
    P = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}

    def conv(t, name, relu=True):
        w = P[name + ".weight"]
        t = F.conv2d(t, w, P[name + ".bias"], padding=w.shape[-1] // 2)
        return torch.relu(t) if relu else t

    with torch.no_grad():
        t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
        for v in O.VGG:
            t = F.max_pool2d(t, 2, 2) if v == "pool" else conv(t, v[0])
        out1 = t
        br = {}
        for b in ("L1", "L2"):
            u = out1
            for name in ("conv5_1_CPM", "conv5_2_CPM", "conv5_3_CPM", "conv5_4_CPM"):
                u = conv(u, f"{name}_{b}")
            br[b] = conv(u, f"conv5_5_CPM_{b}", relu=False)
        for s in range(2, 7):
            cat = torch.cat([br["L1"], br["L2"], out1], 1)
            nxt = {}
            for b in ("L1", "L2"):
                u = cat
                for j in range(1, 7):
                    u = conv(u, f"Mconv{j}_stage{s}_{b}")
                nxt[b] = conv(u, f"Mconv7_stage{s}_{b}", relu=(s == 6 and b == "L2"))
            br = nxt
        return torch.cat([br["L1"], br["L2"]], 1)[0].permute(1, 2, 0).numpy()
