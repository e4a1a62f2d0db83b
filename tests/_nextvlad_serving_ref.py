"""Float64 / host restatements for serving the NeXtVLAD family, on top of tests/_nextvlad_distill_ref.py: what a served
grid tower predicts (the evaluation forward on the checkpoint's moving statistics), with the rows of videos that have no frame zeroed as
the compacting graph hands them out, and the frames a NeXtVLAD cascade stage reads."""
import numpy as np

import _nextvlad_distill_ref as dx


def served_fwd(xn, n, every_n, P, M, zero_empty=False, num_mixtures=2):
    """(predictions [B, V], state [B, H]) of a served grid tower: dx.nextvlad_packed_eval_fwd; zero_empty: rows of videos with n <= 0
    are zeros (NeXtVladEvalGraph(compact=True))."""
    pred, state, _ = dx.nextvlad_packed_eval_fwd(xn, n, every_n, P, M, num_mixtures)
    if zero_empty:
        empty = np.asarray(n).reshape(-1) <= 0
        pred, state = pred.copy(), state.copy()
        pred[empty], state[empty] = 0.0, 0.0
    return pred, state


def stage_frames(n, active, every_n, max_frames):
    """Frames a NeXtVLAD stage reads: sum over its active rows of ceil(min(n_b, max_frames) / every_n), one video at a time."""
    n = np.asarray(n).reshape(-1)
    act = np.ones(n.shape[0], bool) if active is None else np.asarray(active).reshape(-1) != 0
    return sum(-(-min(int(nb), max_frames) // every_n) for nb, a in zip(n, act) if a and nb > 0)


def split_params(state_dict, scope):
    """(variables, moving statistics) of one tower of a TF-named state dict, as float64 numpy without the scope prefix."""
    pre = scope + "/"
    P = {k[len(pre):]: v.detach().cpu().double().numpy() for k, v in state_dict.items() if k.startswith(pre) and hasattr(v, "detach")}
    M = {k: P.pop(k) for k in list(P) if "/moving_" in k}
    P.pop("adam", None)
    return P, M
