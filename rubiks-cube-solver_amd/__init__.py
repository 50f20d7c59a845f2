"""MI355X-native vectorised Rubik's-cube environment (gfx950 HIP kernels behind a C ABI).

Drop-in surface for the env path of SUNGBEOMCHOI/Rubiks-Cube-Solver:
  make_env / CubeEnv  (env.py:3-5, gym-cube/gym_cube/envs/cube_env.py)   batch-1 facade
  VecCubeEnv                                                            the batched env
  TensorReplayBuffer  (utils.py:203-270 ReplayBuffer)                   device-resident sink of ADI samples
  get_env_config      (utils.py:162-186)
  CodeNet             the reference's DeepCube (model.py:7-45) evaluated from compact codes: no dense one-hot, HIP first layer
  ops                 batched operator layer (assets/py333.py:211-246)
  CornerTable         exact distances of the corner states on the device (pattern.py): God's algorithm on the 2x2x2, the admissible corner
                      bound on the 3x3x3; search.* take it with front="table"
  EdgeTable, MaxTable exact distances of up to 7 tracked edge pieces of the 3x3x3 (pattern.py), and the maximum of a corner table and edge
                      tables: the stronger admissible bound front="table" takes in a CornerTable's place
  ChainTables         the four coset-distance tables of Thistlethwaite's subgroup chain (pattern.py), and chain_solve, the descent through
  chain_solve         them (search.py): a solution of ANY legal 3x3x3 in at most 87 quarter turns, no net, no search
  ida_search          Korf's IDA* under those pattern databases (search.py): the OPTIMAL solution of a 3x3x3, no node pool
  TwoPhaseTables      the four coset tables of Kociemba's two-phase algorithm (pattern.py), and two_phase_solve (search.py): a SHORT
  two_phase_solve     solution of ANY legal 3x3x3 -- never longer than chain_solve's -- by two table-guided depth-first searches
  relative_to, two_phase_solve_both, random_state_scramble, invert_actions   the cube group's tie-ins (search.py): solve to a goal other
                      than solved, solve the cube and its inverse and keep the shorter answer, random-state scrambles from uniformly
                      drawn cubes (ops.group_product / group_inverse / random_cubies; VecCubeEnv.compose / invert / reset_uniform)
  get_cubies, RCC_*   the cube as pieces: (piece, orientation) bytes, the legality status bits, perfect indices (ops.cubies / from_cubies)
  py333               the same operators under the reference's names, one cube per call
  py222               the six names cube_env.py:8 imports from the file the reference does not ship (2x2x2, one cube per call)
The directory is named `rubiks-cube-solver_amd`; import it as `rubiks_cube_solver_amd`.
"""
from .tables import (ACTION_NAMES, RCC_BAD_COLOUR, RCC_BAD_FIXED, RCC_BAD_PIECE, RCC_DUP_PIECE, RCC_FLIP, RCC_NAMES, RCC_PARITY,  # noqa: F401
                     RCC_TWIST, get_cubies, get_env_config, get_tables)

__all__ = ["get_env_config", "get_tables", "get_cubies", "ACTION_NAMES", "RCC_BAD_COLOUR", "RCC_BAD_FIXED", "RCC_BAD_PIECE", "RCC_DUP_PIECE",
           "RCC_TWIST", "RCC_FLIP", "RCC_PARITY", "RCC_NAMES", "ops", "make_env", "CubeEnv", "VecCubeEnv", "TensorReplayBuffer", "CodeNet", "CornerTable", "EdgeTable",
           "MaxTable", "ChainTables", "chain_solve", "ida_search", "TwoPhaseTables", "two_phase_solve", "relative_to",
           "two_phase_solve_both", "random_state_scramble", "invert_actions"]


def __getattr__(name):  # torch-dependent parts load lazily
    import importlib

    if name in ("ops", "_lib", "vec_env", "cube_env", "adi", "mcts_batched", "rollout", "dist", "py333", "py222", "replay", "search", "codenet", "pattern"):
        return importlib.import_module(f"{__name__}.{name}")
    if name == "VecCubeEnv":
        return importlib.import_module(f"{__name__}.vec_env").VecCubeEnv
    if name == "TensorReplayBuffer":
        return importlib.import_module(f"{__name__}.replay").TensorReplayBuffer
    if name == "CodeNet":
        return importlib.import_module(f"{__name__}.codenet").CodeNet
    if name in ("CornerTable", "EdgeTable", "MaxTable", "ChainTables", "TwoPhaseTables"):
        return getattr(importlib.import_module(f"{__name__}.pattern"), name)
    if name in ("chain_solve", "ida_search", "two_phase_solve", "relative_to", "two_phase_solve_both", "random_state_scramble", "invert_actions"):
        return getattr(importlib.import_module(f"{__name__}.search"), name)
    if name in ("CubeEnv", "make_env"):
        return getattr(importlib.import_module(f"{__name__}.cube_env"), name)
    raise AttributeError(name)
