"""Shared synthetic-input recipe for tests; mirrors tests/golden/make_golden.py."""
import os

import numpy as np
import torch

from oracle import weights as W

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
SMALL = W.default_dims(max_seq_len=24, L=32, NL=2, F=64, Te=64, Dt=32, Nt=8)
FULL = W.default_dims()
SMALL_SEED = 2
CTRL = W.default_dims(max_seq_len=24, L=32, NL=3, F=64, Te=64, Dt=32, Nt=8)
CTRL_COPY, CTRL_FEATS, CTRL_TC = 2, 35, 20
HML_SMALL = W.humanml3d_dims(max_seq_len=24, L=32, NL=2, F=64, Te=64, Dt=32, Nt=8)
KIT_SMALL = W.humanml3d_dims(max_seq_len=24, L=32, NL=2, F=64, Te=64, Dt=32, Nt=8, input_feats=251, dataset='kit_ml')
HML_FULL = W.humanml3d_dims()          # reference configs/stmogen/T2M_humanml3d.py architecture


def synth_inputs(dims, B, T, seed, lengths=None):
    g = torch.Generator().manual_seed(seed)
    x_T = torch.randn(B, T, dims['input_feats'], generator=g)
    xf = torch.nn.functional.layer_norm(torch.randn(B, dims['Nt'], dims['Dt'], generator=g), (dims['Dt'],))
    mask = torch.ones(B, T)
    if lengths is not None:
        for b, n in enumerate(lengths):
            mask[b, n:] = 0
    return x_T, xf, mask


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def step_noise_from_seed(seed, shape, num):
    """The per-step randn_like stream of the reference loop under torch.manual_seed(seed)."""
    g = torch.Generator().manual_seed(int(seed))
    return [torch.randn(shape, generator=g) for _ in range(num)]


# ---- MoE routing references (tests/test_moe_skew.py; pinned against tutel_restated in tests/test_oracle.py) ---------------
def key_bits(key):
    """Importance keys as uint32 numpy bits: a float tensor / array is taken as fp32 values, an integer one as their bits."""
    if not torch.is_tensor(key):
        a = np.asarray(key).reshape(-1)
        return a.astype(np.float32).view(np.uint32) if a.dtype.kind == 'f' else a.astype(np.uint32)
    k = key.detach().cpu().reshape(-1)
    if k.is_floating_point():
        k = k.float().contiguous().view(torch.int32)
    return k.to(torch.int32).numpy().view(np.uint32)


def bpr_keep(idx, key, E, capacity, tie='stable'):
    """Keep flags [N, 2] (bool numpy) of tutel's batch-prioritised top-2 routing, from a kernel's own expert ids ``idx``
    [N, 2] and importance keys ``key`` [N] (fp32 bits of each token's top score; positive scores, so the bits order like
    the values).  Tokens rank by key descending, then token index ascending ('stable') or descending ('reverse').  Choice
    0 of expert e keeps its first ``capacity`` tokens in that order; choice 1 keeps its first ``capacity - count0[e]``,
    with count0[e] the number of first choices of e before any drop (none when that limit is <= 0).  Exact integer
    arithmetic: the same decision as ``tutel_restated.extract_critical``'s ``locations < capacity``."""
    idx = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).reshape(-1, 2).astype(np.int64)
    kb = key_bits(key).astype(np.uint64)
    N = idx.shape[0]
    assert kb.shape[0] == N, (kb.shape, N)
    assert tie in ('stable', 'reverse'), tie
    tok = np.arange(N, dtype=np.uint64)
    comp = (kb << np.uint64(32)) | (tok ^ np.uint64(0xFFFFFFFF) if tie == 'stable' else tok)    # all distinct
    rank = np.empty(N, dtype=np.int64)
    rank[np.argsort(comp, kind='stable')[::-1]] = np.arange(N)          # 0 = most important
    count0 = np.bincount(idx[:, 0], minlength=E)
    keep = np.empty((N, 2), dtype=bool)
    for k in range(2):
        e = idx[:, k]
        s = np.argsort(e * N + rank, kind='stable')                      # by expert, then by rank
        start = np.concatenate(([0], np.cumsum(np.bincount(e, minlength=E))))
        pos = np.empty(N, dtype=np.int64)
        pos[s] = np.arange(N) - start[e[s]]                              # rank among the tokens of the same (choice, expert)
        limit = capacity if k == 0 else capacity - count0[e]
        keep[:, k] = pos < limit
    return keep


def _gate_keys(l):
    return f'temporal_decoder_blocks.{l}.ca_block.motion_moe.model.gates.0.'


def skew_gates(sd, dims, kind, seed=0):
    """A copy of state dict ``sd`` whose motion-MoE gates route like a trained checkpoint rather than random weights; only
    each base layer's ``gates.0.{cosine_projector.*, sim_matrix, temperature}`` change.

    'hot_pair': a strong common projector bias along a direction u, two sim_matrix columns aligned with u (and split
      by a second direction v that the token-dependent part of the projection sees with either sign), two columns
      anti-aligned, the temperature at its clamp (logit scale 100): two experts take most first AND second choices, so
      they overflow, their second choices are cut wholesale (limit <= 0) and several experts stay empty.
    'all_ties': cosine_projector.weight = 0, so every token has bit-identical scores: one expert takes every first
      choice, another every second one, the other experts get nothing, and only the token index orders the capacity cut.
    'balanced': ``sd`` unchanged (the control)."""
    out = dict(sd)
    if kind == 'balanced':
        return out
    E = dims['E']
    for l in range(dims['NL']):
        pre = _gate_keys(l)
        g = torch.Generator().manual_seed(1000 * seed + 17 + l)
        w = sd[pre + 'cosine_projector.weight']
        if kind == 'all_ties':
            out[pre + 'cosine_projector.weight'] = torch.zeros_like(w)
            out[pre + 'cosine_projector.bias'] = torch.randn(w.shape[0], generator=g)
            continue
        assert kind == 'hot_pair', kind
        P = w.shape[0]
        q, _ = torch.linalg.qr(torch.randn(P, 2, generator=g, dtype=torch.float64))
        u, v = q[:, 0], q[:, 1]
        # the token-dependent part W z has a norm of ~sqrt(P) at these weights: a bias of HOT_BIAS * sqrt(P) along u leaves
        # a fraction of each token's direction free to pick among the others
        out[pre + 'cosine_projector.bias'] = (sd[pre + 'cosine_projector.bias'].double() + HOT_BIAS * P ** 0.5 * u).float()
        wv = w.double() + HOT_V * (v[:, None] * torch.randn(1, w.shape[1], generator=g, dtype=torch.float64)) / w.shape[1] ** 0.5
        out[pre + 'cosine_projector.weight'] = wv.float()
        sim = sd[pre + 'sim_matrix'].double().clone()
        sim = sim / sim.norm(dim=0, keepdim=True)                        # unit columns: random directions
        hot = torch.randperm(E, generator=g)[:4]
        sim[:, hot[0]] = u + HOT_SPLIT * v
        sim[:, hot[1]] = u - HOT_SPLIT * v
        sim[:, hot[2]] = -u                                              # never chosen: empty experts
        sim[:, hot[3]] = -u + 0.1 * v
        out[pre + 'sim_matrix'] = (0.01 * sim).float()
        out[pre + 'temperature'] = torch.full_like(sd[pre + 'temperature'], HOT_TEMP)
    return out


HOT_BIAS, HOT_V, HOT_SPLIT, HOT_TEMP = 0.35, 0.5, 0.3, 3.0        # tuned on the CPU oracle (B = 2 .. 8 at 196 frames)


# ---- evaluation-side fixtures (shared with tests/golden/make_golden.py) -----------------------------------------
EVAL_DIMS = dict(nfeats=322, latent_dim=128, ff_size=256, num_layers=2, num_heads=2)
EVAL_BERT = dict(dim=128, n_layers=2, n_heads=2, hidden_dim=256, max_position_embeddings=64)
T2M_DIMS = dict(input_size=263, movement_hidden_size=64, movement_latent_size=64, motion_hidden_size=128, motion_latent_size=32)
T2M_TEXT = dict(word_size=300, pos_size=15, hidden_size=64, output_size=32)


class StubEvalModel:
    """Deterministic stand-in for the embedding model so that the evaluators' host logic can be compared end to end."""
    device = 'cpu'

    def __init__(self, nfeats=12, d=16):
        g = torch.Generator().manual_seed(5)
        self.P = torch.randn(nfeats, d, generator=g)

    def encode_motion(self, motion, motion_length=None, motion_mask=None, **kw):
        m = motion_mask[..., None].to(motion.dtype)
        return torch.tanh(((motion * m).sum(1) / motion_length[:, None].to(motion.dtype)) @ self.P)

    def encode_text(self, text, token=None, device=None, **kw):
        v = torch.tensor([[float(ord(c) % 13) for c in (t + ' ' * 12)[:12]] for t in text])
        return torch.tanh((v - 6.0) / 4.0 @ self.P[:12])

    def to(self, device):
        return self

    def eval(self):
        return self


def _stub_results(n, nfeats=12, seed=9, T=14):
    """results as the test loop collects them: every motion padded to the dataset's fixed T with a length mask (the
    reference's own prepare_results cannot pad the ground-truth side: base_evaluator.py:75 calls type_as on a list)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        n_i = int(torch.randint(6, T + 1, (1,), generator=g))
        msk = (torch.arange(T) < n_i).float()
        mot = torch.randn(T, nfeats, generator=g) * msk[:, None]
        out.append(dict(motion=mot, pred_motion=mot + 0.7 * torch.randn(T, nfeats, generator=g) * msk[:, None], motion_mask=msk,
                        pred_motion_mask=msk, motion_length=torch.tensor(n_i), pred_motion_length=torch.tensor(n_i),
                        text=''.join(chr(97 + int(c)) for c in torch.randint(0, 26, (10,), generator=g)), token=None))
    return out


def stub_eval_results(n, replications, append_indexes):
    """Result list in the layout the evaluators slice: per replication, n samples followed by the MultiModality repeats
    (fresh predictions for the re-drawn indexes)."""
    out = []
    for rep in range(replications):
        base = _stub_results(n, seed=9 + rep)
        g = torch.Generator().manual_seed(100 + rep)
        extra = []
        for i in append_indexes[rep]:
            r = dict(base[int(i)])
            r['pred_motion'] = r['motion'] + 0.7 * torch.randn(r['motion'].shape, generator=g) * r['motion_mask'][:, None]
            extra.append(r)
        out += base + extra
    return out
