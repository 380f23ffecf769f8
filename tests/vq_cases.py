"""The small cases the quantiser-kind tests share (tests/ only; imports the oracle): golden model A's geometry with each kind of
quantiser, seeded codebooks whose assignments are safe from fp32 rounding (the margin condition), the oracle's composition
encoder -> quantiser -> decoder per kind, and the float64 restatement of the sliced list statistics."""
import numpy as np
import torch

from helpers import golden_model
from oracle import wae_oracle as O

BETA, DECAY = 0.25, 0.9
# Geometry keys per kind, on model A (Cc 16, K 32).  "sliced" takes a second codebook of another size, as SlicedVectorQuantize(K1=).
KINDS = {
    "sliced": dict(vq="sliced", vq_slices=2, K1=20),
    "ema": dict(vq="ema", vq_decay=DECAY),
    "sliced_ema": dict(vq="sliced_ema", vq_slices=2, vq_decay=DECAY),
}
LIST_KINDS = {
    "sliced2": dict(vq="sliced", vq_slices=2, K1=20),
    "sliced4": dict(vq="sliced", vq_slices=4),
    "sliced_ema": dict(vq="sliced_ema", vq_slices=2, vq_decay=DECAY),
}
SEED = 0          # codebook seed; test_vq_kinds_cpu.py asserts the margin condition for it
MARGIN = 1e-4     # least top-2 distance gap, as a fraction of the slice's largest distance (float64)


def slice_specs(cfg):
    """(suffix, d0, D, K) per slice, written out from the reference's constructors (not from packing.py)"""
    kind, Cc, K = cfg.get("vq", "plain"), cfg["Cc"], cfg["K"]
    if kind in ("plain", "ema"):
        return [("", 0, Cc, K)]
    n = cfg.get("vq_slices", 2)
    D = Cc // n
    return [(str(s + 1), s * D, D, cfg["K1"] if (s == 1 and cfg.get("K1") is not None) else K) for s in range(n)]


def coeffs(kind, beta=BETA):
    """(c_loss, has codebook gradient) per kind: vector_quantization.py:41-43, :113-118, :220, :294"""
    return {"plain": (1.0 + beta, True), "sliced": (1.0 + beta, True), "ema": (beta, False), "sliced_ema": (beta, False)}[kind]


def codebooks(cfg, spread, seed=SEED):
    """uniform codebooks of 1.5 x the latents' spread, one generator per (seed, slice)"""
    out = {}
    for sfx, _, D, K in slice_specs(cfg):
        gen = torch.Generator().manual_seed(1000 * seed + len(out))
        out[f"vq.embedding{sfx}.weight"] = (torch.rand(K, D, generator=gen) * 2 - 1) * 1.5 * spread
    return out


def model_case(kind_cfg, seed=SEED):
    """-> (cfg, sd, inputs, ocfg): model A with the kind's codebooks (and zero EMA statistics) in the place of vq.embedding.weight"""
    cfg, sd, ins, _, ocfg = golden_model("A")
    cfg = dict(cfg, **kind_cfg)
    with torch.no_grad():
        lat = O.encoder_forward(sd, ins["c"])
    sd = {k: v for k, v in sd.items() if not k.startswith("vq.")}
    sd.update(codebooks(cfg, float(lat.abs().max()), seed))
    if cfg["vq"] in ("ema", "sliced_ema"):
        for sfx, _, D, K in slice_specs(cfg):
            sd[f"vq.ema_cluster_size{sfx}"] = torch.zeros(K)
            sd[f"vq.ema_w{sfx}"] = torch.zeros(K, D)
    return cfg, sd, ins, ocfg


def is_buffer(key):
    return key.startswith("vq.ema_")


def worst_margin(cfg, sd, lat):
    """least top-2 gap over every frame and slice, as a fraction of the slice's largest distance, in float64"""
    worst = np.inf
    for sfx, d0, D, _ in slice_specs(cfg):
        dis = O.vq_distances(sd[f"vq.embedding{sfx}.weight"].double(), lat[:, d0:d0 + D].double())
        if dis.shape[1] < 2:
            continue
        top2 = torch.topk(dis, 2, dim=1, largest=False).values
        worst = min(worst, float((top2[:, 1] - top2[:, 0]).min() / dis.abs().max()))
    return worst


def quantise(cfg, sd, lat, training=False, beta=BETA):
    """the oracle's quantiser of the kind on latents (B, Cc, Tq) -> (quant, vq_loss, perp, [idx per slice], new state | None)"""
    kind = cfg["vq"]
    if kind == "sliced":
        q, loss, perp, idx = O.sliced_vq_forward(sd["vq.embedding1.weight"], sd["vq.embedding2.weight"], lat, beta)
        return q, loss, perp, list(idx), None
    sfxs = [s for s, _, _, _ in slice_specs(cfg)]
    state = {}
    for s in sfxs:
        state.update({"embedding" + s: sd[f"vq.embedding{s}.weight"], "ema_cluster_size" + s: sd["vq.ema_cluster_size" + s],
                      "ema_w" + s: sd["vq.ema_w" + s]})
    fn = O.vq_ema_forward if kind == "ema" else O.sliced_vq_ema_forward
    q, loss, perp, idx, new = fn(state, lat, beta, cfg.get("vq_decay", 0.99), training)
    out = {}
    for s in sfxs:
        out.update({f"vq.embedding{s}.weight": new["embedding" + s], "vq.ema_cluster_size" + s: new["ema_cluster_size" + s],
                    "vq.ema_w" + s: new["ema_w" + s]})
    return q, loss, perp, list(idx) if isinstance(idx, (tuple, list)) else [idx], out


def oracle_forward(cfg, sd, ocfg, xin, c, g, training=False):
    """encoder -> the kind's quantiser -> decoder, every piece the oracle's -> (logits, vq_loss, perp, aux)"""
    lat = O.encoder_forward(sd, c)
    q, loss, perp, idx, new = quantise(cfg, sd, lat, training)
    y = O.wavenet_forward(sd, ocfg, xin, q, g)
    return y, loss, perp, dict(latents=lat, quant=q, idx=idx, state=new)


def list_stats_f64(cfg, lat, quant, idx, beta=BETA):
    """float64 restatement of one utterance's list statistics: lat, quant (Cc, Tq), idx (n, Tq) or (Tq,) ->
    (vq_loss = c_loss sum_s sqerr_s / (Tq Dtot), perp = sum_s perp_s, hist (n, max K_s), [sqerr_s])"""
    specs = slice_specs(cfg)
    idx = np.asarray(idx).reshape(len(specs), -1)
    lat, quant = np.asarray(lat, dtype=np.float64), np.asarray(quant, dtype=np.float64)
    Tq = lat.shape[1]
    hist = np.zeros((len(specs), max(K for _, _, _, K in specs)), dtype=np.int64)
    sq, perp = [], 0.0
    for s, (_, d0, D, K) in enumerate(specs):
        sq.append(float(((quant[d0:d0 + D] - lat[d0:d0 + D]) ** 2).sum()))
        hist[s, :K] = np.bincount(idx[s], minlength=K)
        p = hist[s, :K] / Tq
        perp += float(np.exp(-np.sum(p * np.log(p + 1e-10))))
    return coeffs(cfg["vq"], beta)[0] * sum(sq) / (Tq * lat.shape[0]), perp, hist, sq
