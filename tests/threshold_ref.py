"""The yardstick of the threshold tests: the window rule as written, (t >= mn) & (t <= mx), on whole tables, one window
at a time, and what the merge-side kernels tally from those masks.  The expressions are torch's so that 765 windows over
up to 33 tables of 2^19 bytes take a fraction of a second where the tables already are (numpy needs 10^10 byte compares
for the same); on the CPU the same functions are checked against the numpy yardsticks in test_segment_ref_host.py."""
import numpy as np
import torch


def stack(tabs, device):
    """(N, n) uint8 tensor of host tables."""
    return torch.from_numpy(np.stack(tabs)).to(device)


def masks(T, mn, mx):
    """(N, n) bool: the window rule, nothing else."""
    return (T >= mn) & (T <= mx)


def pair(m):
    """(N, N) uint64 numpy: addresses where tables i and j are both valid, i <= j; 0 below the diagonal."""
    both = (m[:, None, :] & m[None, :, :]).sum(dim=2)
    return torch.triu(both).cpu().numpy().astype(np.uint64)


def patterns(m):
    """(2^N,) uint64 numpy: the addresses per presence pattern."""
    N = m.shape[0]
    words = (m.to(torch.int64) << torch.arange(N, device=m.device)[:, None]).sum(dim=0)
    return torch.bincount(words, minlength=1 << N).cpu().numpy().astype(np.uint64)


def selection(m_present, T_absent, min_present, max_absent):
    """(n,) bool: p(x) >= min_present and q(x) <= max_absent, q counting the absent tables that hold anything."""
    p = m_present.sum(dim=0)
    q = (T_absent >= 1).sum(dim=0) if T_absent.shape[0] else torch.zeros_like(p)
    return (p >= min_present) & (q <= max_absent)


def table(T_present, m_present, sel, op):
    """(n,) uint8 tensor: `op` (sum clamped to 255, or count) over the present bytes inside the window, 0 where not selected."""
    if op == "sum":
        r = (T_present.to(torch.int64) * m_present).sum(dim=0).clamp(max=255)
    elif op == "count":
        r = m_present.sum(dim=0)
    else:
        raise ValueError(op)
    return (r * sel).to(torch.uint8)
