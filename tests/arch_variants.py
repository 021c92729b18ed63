"""Cell genotypes and network level paths other than the shipped SceneFlow architecture, shared
by the tests that run the executors on them (tests/test_gpu_arch_variants.py, the seeded sweep of
tests/test_executor_plan_cpu.py) and by tools/gen_golden_arch.py, which pins the oracle on them.

Genotype rows are (branch, primitive) in the file's order (genotypes_2d.py / genotypes_3d.py):
primitive 1 is the 3x3 conv, 0 is skip_connect; with three steps the branches of step 0 are 0-1,
of step 1 2-4, of step 2 5-8 (branch - offset = the state read).  ``None`` stands for the shipped
file."""
import numpy as np

STEP_BRANCHES = ((0, 1), (2, 3, 4), (5, 6, 7, 8))

MATCHING_GENOTYPES = {
    "shipped": None,
    "with_skip": [[1, 1], [0, 1], [3, 1], [4, 0], [8, 1], [6, 1]],          # a skip term inside a cell
    "seven_convs": [[0, 1], [1, 1], [2, 1], [3, 1], [6, 1], [7, 1], [8, 1]],  # three-term steps; s1 group of 3
    "no_s1_group": [[0, 1], [1, 1], [2, 1], [4, 1], [5, 1], [7, 1]],        # two convs per step, no group
    "skip_only_state": [[0, 0], [1, 1], [2, 0], [4, 0], [5, 1], [6, 1]],    # a state made by copy_/add_ alone
    "s1_last": [[0, 1], [2, 1], [4, 1], [6, 1], [8, 1]],                    # one op per step
}

# cells 1, 4 and 8 stay at level 1 (conv1 / conv2 concatenate their outputs, skip_model_3d.py:150,155)
MATCHING_PATHS = {
    "shipped": None,
    "end0": [1, 1, 2, 2, 1, 2, 2, 2, 1, 0, 0, 0],
    "start0_end2": [0, 1, 2, 2, 1, 1, 2, 2, 1, 2, 2, 2],
    "end3": [1, 1, 2, 2, 1, 2, 3, 2, 1, 2, 3, 3],
    "up_then_down_L1": [1, 1, 2, 2, 1, 2, 2, 2, 1, 2, 1, 2],
    "zigzag": [1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1],
}

FEATURE_GENOTYPES = {
    "shipped": None,
    "group_covers_pair": [[0, 1], [1, 1], [3, 1], [4, 1], [5, 1], [8, 1]],
    "skips_and_group": [[0, 1], [1, 0], [3, 1], [4, 1], [5, 1], [6, 1]],
    "skip_only_state": [[0, 1], [3, 0], [4, 0], [5, 1], [6, 1]],
    "three_terms": [[0, 1], [1, 1], [2, 0], [3, 0], [4, 1], [5, 0]],
    "one_branch": [[1, 1], [2, 1], [3, 1], [7, 1]],
}

FEATURE_PATHS = {"shipped": None, 1: [1, 1, 0, 1, 1, 1], 2: [1, 2, 2, 1, 2, 2], 3: [1, 2, 3, 3, 2, 3]}

# what MatchingExecutor plans per level path, worked out from the path's level changes d[i]
# (-1 down, 0 same, 1 up): `share` at a cell that changes level followed by one that does not
# (d[i] != 0, d[i + 1] == 0); `fanout` at the other cells that do not read their s1 down-sampled
# and whose successor reads the same source no lower than that (d[i] >= 0, d[i] + d[i + 1] >= 0);
# conv1 writes cell 5's level where cell 5 has a `share` and goes down; the stems write cell 0's
# where cell 0 goes down
PLANNED = {
    "shipped": dict(share={0, 2, 5, 8}, fanout={3, 4, 6, 7, 9, 10}, conv1_down=True, cell0_down=True),
    "end0": dict(share={0, 2, 5, 9}, fanout={3, 4, 6, 7, 8, 10}, conv1_down=True, cell0_down=True),
    "start0_end2": dict(share={2, 4, 6, 9}, fanout={3, 7, 8, 10}, conv1_down=False, cell0_down=False),
    "end3": dict(share={0, 2, 10}, fanout={3, 4, 7, 8}, conv1_down=False, cell0_down=True),
    "up_then_down_L1": dict(share={0, 2, 5}, fanout={3, 4, 6, 7, 8, 10}, conv1_down=True, cell0_down=True),
    "zigzag": dict(share={0, 3, 6}, fanout={1, 2, 4, 5, 7, 8, 9, 10}, conv1_down=False, cell0_down=True),
}
# (genotype, path) for which _cell_output_takes_down(10, .) holds at a volume that halves
CELL10_DOWN_GENOTYPES = ("shipped", "seven_convs", "no_s1_group", "s1_last")
CELL10_DOWN_PATHS = ("shipped", "up_then_down_L1", "zigzag")


def random_genotype(rng, shuffle=False):
    """A legal genotype: every step draws 1-3 of its branches and a random primitive per row.
    Rows by ascending branch, or (``shuffle``) in a random order within the step: the cells pair
    the k-th row's op with the k-th matched branch in ascending order (Cell.forward :57-68)."""
    rows = []
    for branches in STEP_BRANCHES:
        n = int(rng.integers(1, min(3, len(branches)) + 1))
        picked = sorted(rng.choice(branches, size=n, replace=False).tolist())
        if shuffle:
            picked = rng.permutation(picked).tolist()
        rows += [[int(b), int(rng.integers(0, 2))] for b in picked]
    return rows


def arch_with(base, fea_geno=None, fea_path=None, mat_geno=None, mat_path=None):
    """The four arrays of an architecture: ``base`` (the shipped ones, golden_util.arch()) with the
    named (or literal) variants put in."""
    def pick(table, v):
        return table[v] if isinstance(v, (str, int)) else v
    a = dict(base)
    for key, table, v in (("cell_arch_fea", FEATURE_GENOTYPES, fea_geno), ("net_arch_fea", FEATURE_PATHS, fea_path),
                          ("cell_arch_mat", MATCHING_GENOTYPES, mat_geno), ("net_arch_mat", MATCHING_PATHS, mat_path)):
        v = pick(table, v)
        if v is not None:
            a[key] = np.array(v)
    return a
