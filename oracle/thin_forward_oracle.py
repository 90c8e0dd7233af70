"""Host restatement of what hb_thin_forward (csrc/learner2.hip, thin_forward_kernel) must and may write, and of the two host
formulas its launch is sized by. TEST INFRASTRUCTURE ONLY; plain numpy, no arithmetic of the product itself (the values come from
oracle/actor_oracle.py thin_gemm).

Contract (include/hanabi_hip.h): the 2B operand rows are {obs_tm1 [0, B), obs_t [B, 2B)}.
  layer 1  out [2B, n], n = 2 * hidden = [online | target] columns: the loss and the backward read every column of the obs_t
           rows and the online half of the obs_tm1 rows; the target network on obs_tm1 is read by nobody.
  layer 2  out [2, 2B, n], entries {online, target}: both entries on the obs_t rows in full; of the online entry on the
           obs_tm1 rows only the K atoms [a K, (a + 1) K) of the action a each sample took; the target entry on obs_tm1 not at all.
The kernel works in 16-column tiles, so it MAY write the tiles that cover what is needed and nothing beyond them."""
import numpy as np

TILE = 16        # columns of one output tile
GROUP = 32       # samples of one gathered row group (two 16-row MFMA tiles)
MAX_WORKGROUPS = 1024


def tiles_touched(start, width):
    """16-column tiles that hold columns [start, start + width)"""
    return (start + width - 1) // TILE - start // TILE + 1


def npair(K):
    """The launch's column tiles per gathered row group: K columns touch at most this many tiles at any alignment."""
    return (K + 14) // 16 + 1


def row_groups(act, A):
    """Row groups the kernel forms: per action, its samples 32 at a time."""
    counts = np.bincount(np.asarray(act, np.int64), minlength=A)
    return int(((counts + GROUP - 1) // GROUP).sum())


def group_bound(B, A):
    """The launch's row groups: B / 32 full ones and at most one partial group per action that occurs."""
    return B // GROUP + min(A, B)


def n_units(layer, B, n, A=0, K=0):
    """Units (32 x 16 output tiles of one product) of a launch; beyond MAX_WORKGROUPS a wavefront walks several."""
    nrt, nct = B // GROUP, n // TILE
    if layer == 1:
        return nrt * (nct // 2) + nrt * nct
    return group_bound(B, A) * npair(K) + 2 * nrt * nct


def workgroups(units):
    """One-wavefront workgroups of a launch: every wavefront walks ceil(units / 1 024) units."""
    per = (units + MAX_WORKGROUPS - 1) // MAX_WORKGROUPS
    return (units + per - 1) // per


def masks(layer, B, n, act=None, A=0, K=0):
    """(need, may): boolean masks over the output, [2B, n] for layer 1 and [2, 2B, n] for layer 2. need: what the loss and the
    backward read; may: need widened to the 16-column tiles that cover it."""
    if layer == 1:
        need = np.zeros((2 * B, n), bool)
        need[B:] = True
        need[:B, :n // 2] = True
    elif layer == 2:
        act = np.asarray(act, np.int64)
        assert act.shape == (B,) and (act >= 0).all() and (act < A).all() and A * K <= n
        cols = np.arange(n)
        need = np.zeros((2, 2 * B, n), bool)
        need[:, B:] = True
        need[0, :B] = (cols[None, :] >= (act * K)[:, None]) & (cols[None, :] < ((act + 1) * K)[:, None])
    else:
        raise ValueError(layer)
    assert n % TILE == 0, "n must be whole tiles"
    may = np.repeat(need.reshape(*need.shape[:-1], n // TILE, TILE).any(-1), TILE, axis=-1)
    return need, may
