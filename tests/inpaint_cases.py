"""Shared by tools/gen_inpaint_golden.py and the inpainting tests: a torch restatement of the reference's LBAMModel forward
(models/inpaint.py:285-357) and Inpainter.__call__ (:17-49), pinned to the reference's own module by the golden
(tests/test_inpaint_model.py), the golden's image and masks, and a synthetic UV layout for the texture case."""
import numpy as np

GOLDEN_HW = (128, 128)


def gauss_a(x, p):
    """GaussActivation.forward with the clamped parameters p = (a, mu, sigma1, sigma2)"""
    a, mu, s1, s2 = p
    left = a * (-s1 * ((x - mu) ** 2)).exp()
    right = 1 + (a - 1) * (-s2 * ((x - mu) ** 2)).exp()
    return left.masked_fill(x >= mu, 0.0) + right.masked_fill(x < mu, 0.0)


def lbam_forward(state, x, mask, dtype=None, pre_tanh=False):
    """LBAMModel(4, 3)(x, mask) in `dtype` (torch.float32 or torch.float64): x [n, 4, H, W], mask [n, 3, H, W] (1 = known).
    pre_tanh=True also returns dc7's output (the tanh argument)."""
    import torch
    import torch.nn.functional as F
    from bodyfitting_amd import inpaint as I
    dtype = dtype or torch.float32
    W = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in state.items()}

    def gp(prefix):
        npd = np.float64 if dtype == torch.float64 else np.float32
        return [torch.tensor(v, dtype=dtype) for v in I.gauss_params(state, prefix, npd)]

    def conv(t, key):
        return F.conv2d(t, W[key], stride=2, padding=1)

    def leaky(t):
        return F.leaky_relu(t, 0.2)

    def mupdate(t):
        return torch.pow(torch.relu(t), 0.8)

    x, mask = torch.as_tensor(x).to(dtype), torch.as_tensor(mask).to(dtype)
    ef, mu, skip, fmap = [], [], [], []
    h, m = x, mask
    for l in range(1, 8):
        c = conv(h, f"ec{l}.conv.conv.weight")
        mm = conv(m, f"ec{l}.conv.maskConv.weight")
        g = gauss_a(mm, gp(f"ec{l}.conv"))
        h, m = leaky(c * g), mupdate(mm)
        ef.append(h); skip.append(c); fmap.append(g)
    rmap = []
    r = 1 - mask
    for l in range(1, 7):
        mm = conv(r, f"reverseConv{l}.reverseMaskConv.weight")
        rmap.append(gauss_a(mm, gp(f"reverseConv{l}")))
        r = mupdate(mm)
    d = ef[6]
    for t in range(1, 7):
        l = 6 - t                                        # skip / forward / reverse maps of encoder level 7 - t (0-based 6 - t)
        up = F.conv_transpose2d(d, W[f"dc{t}.conv.weight"], stride=2, padding=1)
        d = leaky(torch.cat((skip[l], up), 1) * torch.cat((fmap[l], rmap[l]), 1))
    d7 = F.conv_transpose2d(d, W["dc7.weight"], stride=2, padding=1)
    out = (torch.tanh(d7) + 1) / 2
    return (out, d7) if pre_tanh else out


def prepare(image, mask):
    """Inpainter.__call__'s preparation of uint8 [H, W, 3] image and mask -> (x [1, 4, H, W], mask [1, 3, H, W]) float32 torch"""
    import torch
    image = torch.tensor(image, dtype=torch.float32) / 255.
    mask = torch.tensor(mask, dtype=torch.float32) / 255.
    image, mask = image.permute(2, 0, 1), mask.permute(2, 0, 1)
    ones, zeros = mask >= 0.5, mask < 0.5
    mask.masked_fill_(ones, 1.0)
    mask.masked_fill_(zeros, 0.0)
    mask = 1 - mask
    image = image * mask
    H, W = image.shape[1:]
    x = torch.cat((image, mask[0].view(1, H, W)), 0).view(1, 4, H, W)
    return x, mask.view(1, 3, H, W)


def inpaint_forward(state, image, mask, dtype=None):
    """Inpainter(...)(image, mask) with the network in `dtype` -> numpy [H, W, 3] in that dtype"""
    import torch
    x, m = prepare(image, mask)
    dtype = dtype or torch.float32
    x, m = x.to(dtype), m.to(dtype)
    with torch.no_grad():
        out = lbam_forward(state, x, m, dtype)
    out = out * (1 - m) + x[:, 0:3] * m
    return out[0].permute(1, 2, 0).numpy()


def golden_image(H=128, W=128, seed=3):
    """a smooth synthetic BGR texture with grey (128) patches"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([127 + 100 * np.sin(xx / 9 + c) * np.cos(yy / 13 - c) for c in range(3)], -1)
    img += rng.normal(0, 2, img.shape)
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[H // 8:H // 8 + H // 5, W // 6:W // 6 + W // 4] = 128
    img[H // 2:H // 2 + H // 6, W // 2:W // 2 + W // 3] = 125
    return img


def masks(H, W, seed=5):
    """name -> uint8 [H, W, 3] mask (255 = hole): empty, full, scattered holes, one large hole; the scattered one has grey
    bytes on both sides of 128 (the threshold) and per-channel differences"""
    rng = np.random.default_rng(seed)
    out = {"empty": np.zeros((H, W, 3), np.uint8), "full": np.full((H, W, 3), 255, np.uint8)}
    s = np.where(rng.random((H, W, 3)) < 0.15, rng.integers(100, 256, (H, W, 3)), rng.integers(0, 128, (H, W, 3)))
    out["scattered"] = s.astype(np.uint8)
    big = np.zeros((H, W, 3), np.uint8)
    big[H // 5:H // 5 + H // 2, W // 4:W // 4 + W // 2 + 7] = 255
    out["large"] = big
    return out


def uv_obj_text(n=24, seed=11):
    """a synthetic UV OBJ (`v`, `vt`, `f v/vt` lines): an n x n grid of quads over [0.02, 0.98]^2, two triangles each, its vt
    jittered -> (text, n_faces)"""
    rng = np.random.default_rng(seed)
    lines = []
    g = np.linspace(0.02, 0.98, n + 1)
    for j in range(n + 1):
        for i in range(n + 1):
            lines.append(f"v {i} {j} 0")
    jit = rng.uniform(-0.3, 0.3, (n + 1, n + 1, 2)) * (g[1] - g[0])
    jit[0, :] = jit[-1, :] = jit[:, 0] = jit[:, -1] = 0
    for j in range(n + 1):
        for i in range(n + 1):
            lines.append(f"vt {g[i] + jit[j, i, 0]:.6f} {g[j] + jit[j, i, 1]:.6f}")
    nf = 0
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i + 1, j * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 2, (j + 1) * (n + 1) + i + 1
            lines.append(f"f {a}/{a} {b}/{b} {c}/{c}")
            lines.append(f"f {a}/{a} {c}/{c} {d}/{d}")
            nf += 2
    return "\n".join(lines) + "\n", nf


def texture_image(H, W, seed=7):
    """a texture map as render_texture_map leaves it: colour, with grey (118 < v < 138 on every channel) regions the fit never
    reached, and pure white"""
    img = golden_image(H, W, seed)
    rng = np.random.default_rng(seed)
    for _ in range(6):
        y, x = rng.integers(0, H - H // 6), rng.integers(0, W - W // 6)
        h, w = rng.integers(H // 12, H // 5), rng.integers(W // 12, W // 5)
        img[y:y + h, x:x + w] = rng.integers(119, 138, 3).astype(np.uint8)
    img[:H // 20, :] = 255
    return img


def golden_out64(z, key="out"):
    """the golden's float64 network result: {key}32 + {key}64_delta (tools/gen_inpaint_golden.py)"""
    return z[key + "32"].astype(np.float64) + z[key + "64_delta"].astype(np.float64)
