"""The nearest-node search strategies the GPU tests select (shared by test_gpu_parity.py and the modules that
import it from there, and by test_walk_index.py)."""


def nn_strategy(pl, name):
    """Select the nearest-node search: 'brute' (node order) or 'walk' (one wave per sample over
    place-ordered tiles, clrrt_nnwalk.hip; the default from 8192 nodes).  'walk_split*':
    the walk with a budget of one tile, so every sample hands its search to the split waves and the
    merge (the overflow path of large trees), 7 waves per sample (odd interleave).  'fused': EXACT lists of
    small trees by one kernel per round (k_nn_exact_fused, the default); every other strategy turns it off
    so that its own path runs."""
    pl.set_option("nn_exact_fused", name == "fused")
    pl.set_option("nn_walk_min", 0 if name.startswith("walk") else 1 << 40)
    # 'coded': the large-tree walk (one log-coded LDS byte per super-tile + the inside-circle key bracket)
    coded = "coded" in name
    pl.set_option("nn_walk_stateless", name.endswith("stateless") or coded)
    pl.set_option("nn_walk_half_max", 0 if coded else 4096)
    # 'persistent': a fixed grid of 1024 walk waves taking samples from per-XCD counters
    pl.set_option("nn_walk_waves", 1024 if "persistent" in name else 0)  # others: one wave per sample
    split = name.startswith("walk_split")
    pl.set_option("nn_walk_budget_tiles", 1 if split else 2048)
    pl.set_option("nn_walk_budget_keys", 1 if split else 4096)
    pl.set_option("nn_walk_chunks", 7 if split else 16)
    pl.set_option("nn_walk_max_over", 1024)
