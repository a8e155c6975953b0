"""Seeded input recipes shared by oracle/make_golden.py (which feeds them to the imported
reference) and the tests (which feed them to the oracle / the HIP path).

numpy's legacy RandomState streams are frozen across numpy versions, so the large inputs
(weights, codebooks, embeddings) are regenerated from seeds instead of being committed; the
golden files under tests/golden/ hold the reference's OUTPUTS (and the few inputs that came
from torch's RNG)."""
import numpy as np

RUN_SH_LAYERS = [2048, 1024, 512, 256, 128, 64]   # reference index/run.sh:15


def rs(seed):
    return np.random.RandomState(seed)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------- F1: RQ known-answer test
def rq_kat(levels, codes, e=32, n=512, seed=100):
    r = rs(seed + levels * 1000 + codes)
    z = f32(r.standard_normal((n, e)))
    cbs = [f32(r.standard_normal((codes, e)) * (0.7 ** l)) for l in range(levels)]
    return z, cbs


# ---------------------------------------------------------------- F2: exact ties
def tie_case(seed=7, n=1024, K=256, e=32):
    """Small integers: every product and partial sum is exact in fp32 in ANY summation order,
    so equal distances are exactly equal and argmin's first-index rule is what is tested."""
    r = rs(seed)
    cb = f32(r.randint(-3, 4, size=(K, e)))
    cb[100] = cb[5]
    cb[200] = cb[5]
    cb[37] = cb[36]
    cb[255] = cb[0]
    z = f32(cb[r.randint(0, K, size=n)] + r.randint(-1, 2, size=(n, e)))
    z[:8] = cb[[5, 100, 200, 36, 37, 0, 255, 5]]       # exact hits on duplicated codes
    z[8] = (cb[10] + cb[11]) / 2                         # exact midpoint (halves are exact in fp32)
    return z, cb


# ---------------------------------------------------------------- F3: Sinkhorn
def sinkhorn_case(B, K=256, seed=300):
    r = rs(seed + B)
    z = f32(r.standard_normal((B, 32)))
    cb = f32(r.standard_normal((K, 32)) * 0.8)
    return z, cb


# ---------------------------------------------------------------- F8: full-size encoder
def encoder_weights(dims, seed=800, bn=False):
    """Xavier-normal-scaled weights (layers.py:33-40 uses xavier_normal_; the draw itself comes
    from numpy here), small non-zero biases, and -- for bn -- random eval-mode statistics."""
    r = rs(seed + dims[0])
    Ws, bs, bns = [], [], []
    nl = len(dims) - 1
    for l in range(nl):
        std = np.sqrt(2.0 / (dims[l] + dims[l + 1]))
        Ws.append(f32(r.standard_normal((dims[l + 1], dims[l])) * std))
        bs.append(f32(0.02 * r.standard_normal(dims[l + 1])))
        if bn and l != nl - 1:
            f = dims[l + 1]
            bns.append(dict(weight=f32(1 + 0.1 * r.standard_normal(f)), bias=f32(0.1 * r.standard_normal(f)),
                            running_mean=f32(0.1 * r.standard_normal(f)),
                            running_var=f32(0.5 + r.uniform(size=f))))
        else:
            bns.append(None)
    return Ws, bs, bns


def encoder_case(in_dim, n, levels=4, codes=256, e=32, bn=False, seed=800):
    dims = [in_dim] + RUN_SH_LAYERS + [e]
    Ws, bs, bns = encoder_weights(dims, seed, bn)
    r = rs(seed + 1 + in_dim + n)
    x = f32(r.standard_normal((n, in_dim)))
    return dims, Ws, bs, bns, x


def fold_bn(bn, eps=1e-5):
    """Eval-mode BatchNorm1d as y = t*scale + shift, computed in fp32 the way the product does."""
    if bn is None:
        return None, None
    scale = f32(bn["weight"] / np.sqrt(bn["running_var"] + np.float32(eps)))
    shift = f32(bn["bias"] - bn["running_mean"] * scale)
    return scale, shift


def state_dict_names(n_layers, bn, levels):
    """State-dict key layout of the reference RQVAE (checkpoint row)."""
    step = 4 if bn else 3
    names = {}
    for part in ("encoder", "decoder"):
        names[part] = [f"{part}.mlp_layers.{l * step + 1}" for l in range(n_layers)]
    names["bn"] = {part: [f"{part}.mlp_layers.{l * step + 2}" for l in range(n_layers - 1)]
                   for part in ("encoder", "decoder")} if bn else {}
    names["codebooks"] = [f"rq.vq_layers.{l}.embedding.weight" for l in range(levels)]
    return names


# ---------------------------------------------------------------- F6: index generation end to end
def toy_items(seed, n=3000, d=128):
    """Clustered toy embeddings with a few exact duplicates (items that can never be separated)."""
    r = rs(seed)
    centres = f32(r.standard_normal((400, d)))
    x = f32(centres[r.randint(0, 400, size=n)] + 0.08 * r.standard_normal((n, d)))
    x[17] = x[5]
    x[1200] = x[5]
    x[2999] = x[2998]
    return x


def toy_checkpoint(directory, cut_last=None):
    """The F6 toy model as a checkpoint on disk, the way the trainer writes one: `directory`/Toy.emb.npy holds toy_items of the
    fixture's seed, `directory`/toy.pth the model arguments of tests/golden/f6_generate.npz (an argparse.Namespace whose data_path
    is that file) and its state dict (the sd__ arrays).  cut_last: the last codebook keeps its first `cut_last` rows only, and
    num_emb_list says so -- with 16 the buckets overflow, so that --spill has work.  Returns (items, path of toy.pth)."""
    import argparse
    import json
    import os

    import torch
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "f6_generate.npz"))
    with open(os.path.join(gold, "manifest.json")) as fh:
        meta = json.load(fh)["fixtures"]["f6_generate.npz"]
    items = toy_items(meta["seed"])
    npy = os.path.join(str(directory), "Toy.emb.npy")
    np.save(npy, items)
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    if cut_last is not None:
        kw["num_emb_list"] = list(kw["num_emb_list"][:-1]) + [cut_last]
        last = state_dict_names(len(kw["layers"]) + 1, kw["bn"], len(kw["num_emb_list"]))["codebooks"][-1]
        sd[last] = sd[last][:cut_last].clone()
    ckpt = os.path.join(str(directory), "toy.pth")
    torch.save({"args": argparse.Namespace(data_path=npy, num_workers=0, **kw), "epoch": 0, "best_loss": 0.0,
                "best_collision_rate": 0.0, "state_dict": sd, "optimizer": {}}, ckpt, pickle_protocol=4)
    return items, ckpt


# ---------------------------------------------------------------- F9: near-tie audit at bench scale
NEARTIE_CASES = {"c3": (1_000_000, 768), "c2": (16_859, 4096)}   # BASELINE.json configs[2], configs[1]


def neartie_items(n, in_dim, seed=900, chunk=65536):
    """[n, in_dim] fp32 N(0,1) items, generated a chunk at a time (PCG64 float32 ziggurat: 768 M values in a
    few seconds).  numpy does not freeze Generator streams across versions, so the fixture stores a sha256 of
    the first chunk and the test refuses to run on a drifted stream instead of reporting false mismatches."""
    g = np.random.Generator(np.random.PCG64(seed + in_dim))
    x = np.empty((n, in_dim), dtype=np.float32)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        x[lo:lo + m] = g.standard_normal((m, in_dim), dtype=np.float32)
    return x


def neartie_encoder(in_dim, e=32, seed=900):
    dims = [in_dim] + RUN_SH_LAYERS + [e]
    Ws, bs, _ = encoder_weights(dims, seed)
    return dims, Ws, bs


# ---------------------------------------------------------------- F10: k-means init (sklearn, host)
def kmeans_case(seed=1000, n=2048, e=32, centres=300):
    """A first-training-batch-sized set of latents with cluster structure (so k-means has something to find)."""
    r = rs(seed)
    c = f32(r.standard_normal((centres, e)))
    return f32(c[r.randint(0, centres, size=n)] + 0.15 * r.standard_normal((n, e)))


# ---------------------------------------------------------------- F11: one training step at the run.sh width
def run_sh_train_case(in_dim=768, batch=1024, e=32, seed=1100):
    """The model index/run.sh trains (MLP 2048-...-64, e 32, BatchNorm -- run.sh's `--bn False` parses as True) with
    Xavier-normal-scaled weights from numpy, BatchNorm affine parameters off 1/0, fresh running statistics, and one
    batch of run.sh's size.  Returns (state dict without codebooks: name -> array, x [batch, in_dim])."""
    dims = [in_dim] + RUN_SH_LAYERS + [e]
    names = state_dict_names(len(dims) - 1, True, 4)
    sd = {}
    for part, d, s in (("encoder", dims, seed), ("decoder", dims[::-1], seed + 7)):
        Ws, bs, bns = encoder_weights(d, s, bn=True)
        for l, nme in enumerate(names[part]):
            sd[nme + ".weight"], sd[nme + ".bias"] = Ws[l], bs[l]
        for l, nme in enumerate(names["bn"][part]):
            f = d[l + 1]
            sd[nme + ".weight"], sd[nme + ".bias"] = bns[l]["weight"], bns[l]["bias"]
            sd[nme + ".running_mean"], sd[nme + ".running_var"] = np.zeros(f, np.float32), np.ones(f, np.float32)
            sd[nme + ".num_batches_tracked"] = np.zeros((), np.int64)
    x = f32(rs(seed + 1).standard_normal((batch, in_dim)))
    return sd, x


def strided_sample(a, limit=2048):
    """The entries of `a` (flattened) a fixture keeps: all of a small tensor, every stride-th of a large one."""
    flat = np.asarray(a).reshape(-1)
    step = max(1, -(-flat.size // limit))
    return flat[::step]


# ---------------------------------------------------------------- the engine's support matrix, one step per configuration
# (tests/test_gpu_support_matrix.py; judged by tests/step_check.py against oracle/torch_ref.py in fp64 -- no fixture)
def _matrix(in_dim, layers, e_dim, codes, bn, loss, batch, sk, beta=0.25, qlw=1.0, dropout=0.0):
    return dict(in_dim=in_dim, layers=layers, e_dim=e_dim, codes=codes, bn=bn, loss=loss, batch=batch, sk=sk, beta=beta,
                qlw=qlw, dropout=dropout)


SUPPORT_MATRIX = {
    "A": _matrix(72, [40, 24], 16, [100, 7, 32], False, "l1", 37, [0.0, 0.0, 0.003]),
    "B": _matrix(128, [72, 40], 64, [64, 48], True, "mse", 50, [0.003, 0.0], beta=0.5, qlw=0.3),
    "C": _matrix(32, [], 32, [16, 16], False, "mse", 2, [0.0, 0.0]),
    "D": _matrix(64, [32], 16, [32, 32, 32], True, "l1", 64, [0.003, 0.003, 0.003], qlw=2.0),
    "E": _matrix(40, [24], 16, [7, 5], False, "mse", 1, [0.0, 0.0]),
    "F": _matrix(136, [264, 72, 40], 32, [256, 100], True, "l1", 131, [0.0, 0.003]),
    "G": _matrix(128, [72, 40], 64, [64, 48], True, "l1", 50, [0.003, 0.0], beta=0.5, qlw=0.3, dropout=0.3),
    "H": _matrix(72, [40, 24], 16, [100, 7, 32], False, "mse", 37, [0.0, 0.0, 0.003], dropout=0.5),
    # two Sinkhorn levels of more than 16 384 batch x codes entries each: the size from which the one-launch solver can
    # give up, so that each level hands the engine a give-up probe (the second one is OR-ed into the flag on its own)
    "I": _matrix(64, [32], 16, [32, 32], True, "mse", 600, [0.003, 0.003]),
}
SUPPORT_MATRIX_SK_ITERS = 50


def near_miss(**changes):
    """The plain model the walk along the edge of the matrix varies one thing of (test_the_edge_of_the_support_matrix)."""
    base = _matrix(64, [32], 16, [32, 32], False, "mse", 48, [0.0, 0.003])
    base.update(changes)
    return base


# the accepted side of that edge: the widths next to 36 and 100 that the kernels do take, the largest e_dim, dropout close to 1
SUPPORT_EDGE = {
    "a": near_miss(layers=[40]), "b": near_miss(layers=[104]), "c": near_miss(in_dim=40), "d": near_miss(in_dim=104),
    "e": near_miss(e_dim=64), "f": near_miss(dropout=0.9),
}


def support_matrix_case(letter, config=None):
    """(configuration, state dict name -> array, batch [rows, in_dim]) of one row of SUPPORT_MATRIX or SUPPORT_EDGE (or of
    `config`, a dict of the same keys, under a letter of its own), all draws from
    RandomState(ord(letter)) in this order: per MLP (encoder, decoder) and layer the Linear weight N(0, 2/(in+out)), its bias
    0.05 N and, in front of a BatchNorm, gamma 1 + 0.1 N and beta 0.1 N (running statistics 0 / 1); the batch N(0, 1); per
    level l the codebook = 0.6**l x rows of the encoder's training-mode latents of the batch (drawn with replacement, no
    dropout) + 0.01 N."""
    import torch
    from oracle import torch_ref
    c = config if config is not None else SUPPORT_MATRIX[letter] if letter in SUPPORT_MATRIX else SUPPORT_EDGE[letter]
    r = rs(ord(letter))
    dims = [c["in_dim"]] + list(c["layers"]) + [c["e_dim"]]
    names = state_dict_names(len(dims) - 1, c["bn"], len(c["codes"]))
    sd = {}
    for part, d in (("encoder", dims), ("decoder", dims[::-1])):
        for l, nme in enumerate(names[part]):
            fan_in, fan_out = d[l], d[l + 1]
            sd[nme + ".weight"] = f32(r.standard_normal((fan_out, fan_in)) * np.sqrt(2.0 / (fan_in + fan_out)))
            sd[nme + ".bias"] = f32(0.05 * r.standard_normal(fan_out))
            if c["bn"] and l != len(dims) - 2:
                bn = names["bn"][part][l]
                sd[bn + ".weight"] = f32(1.0 + 0.1 * r.standard_normal(fan_out))
                sd[bn + ".bias"] = f32(0.1 * r.standard_normal(fan_out))
                sd[bn + ".running_mean"], sd[bn + ".running_var"] = np.zeros(fan_out, np.float32), np.ones(fan_out, np.float32)
                sd[bn + ".num_batches_tracked"] = np.zeros((), np.int64)
    x = f32(r.standard_normal((c["batch"], c["in_dim"])))
    scratch = {k: torch.from_numpy(v.copy()) for k, v in sd.items()}        # (training mode moves the running statistics)
    with torch.no_grad():
        z = torch_ref.mlp(scratch, "encoder", torch.from_numpy(x), len(dims) - 1, c["bn"], training=True).numpy()
    for l, K in enumerate(c["codes"]):
        rows = r.randint(0, c["batch"], size=K)
        sd[names["codebooks"][l]] = f32(0.6 ** l * z[rows] + 0.01 * r.standard_normal((K, c["e_dim"])))
    return c, sd, x
