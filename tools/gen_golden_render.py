#!/usr/bin/env python3
"""Generate the rgb_array golden frames tests/golden/render_<name>.npz from the
REFERENCE's own render().

Runs only in the build container (the reference never travels to the GPU box).  The
fork (`/root/reference/gradio-app/plantos_env_new.py`) is imported through the stubs of
tools/refshim/ (gymnasium, viewers) with tools/refshim_render/pygame in front: a numpy
stand-in for the five generic pygame primitives its sprite-less `_render_frame`
(:697-762) draws with.  `pygame.image.load` raises there, so the reference's own
`except:` selects the colour path.  Nothing from the reference is copied: only the state
arrays and the frames its code returns are written (numpy, allow_pickle=False).

Each fixture holds one state and its frame:
  cfg        i32[5]  grid, plants, obstacles, lidar_range, lidar_channels
  cell_size  i32     env.cell_size (the reference hard-codes 30, :112)
  cells u8[G,G], visits i32[G,G], explored i8[G,G], scalars i32[8]  (pe_get_state terms)
  frame      u8[G*s, G*s, 3]  env.render() with render_mode='rgb_array'

Cases per geometry: a fresh reset; a seeded random rollout; the rover moved into a
corner and onto an edge (ray ends and discs fall off the canvas), onto a plant, beside an
obstacle; a mostly explored map.  Every geometry's set shows both plant kinds.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_render.py
"""
import contextlib
import io
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden")
REF = "/root/reference"

sys.dont_write_bytecode = True
sys.path[:0] = [os.path.join(HERE, "refshim_render"), os.path.join(HERE, "refshim"), REF,
                os.path.join(REF, "gradio-app")]
import plantos_env_new  # noqa: E402  (reference, gradio fork)

ForkEnv = plantos_env_new.PlantOSEnvNew
EMPTY, OBST, HYD, THIRSTY = 0, 1, 2, 3

# name: (grid, plants, obstacles, lidar_range, lidar_channels), cell_size
GEOMETRIES = {
    "g7": ((7, 3, 3, 3, 12), 8),
    "g20": ((20, 10, 12, 6, 16), 6),
    "g21": ((21, 8, 50, 2, 10), 5),   # 315-byte rows
    "g25": ((25, 10, 12, 6, 16), 4),
}


def make(cfg, cell_size):
    G, P, O, R, C = cfg
    env = ForkEnv(grid_size=G, num_plants=P, num_obstacles=O, lidar_range=R, lidar_channels=C,
                  map_generation_algo="original", render_mode="rgb_array")
    env.cell_size = cell_size
    return env


def cells_of(env):
    G = env.grid_size
    c = np.zeros((G, G), np.uint8)
    for (x, y) in env.obstacles:
        c[x, y] = OBST
    for (x, y), t in env.plants.items():
        c[x, y] = THIRSTY if t else HYD
    return c


def move_rover(env, pos):
    """State injection: the rover at `pos` (made a free or plant cell), visited and explored."""
    pos = (int(pos[0]), int(pos[1]))
    env.obstacles.discard(pos)
    ox, oy = env.rover_pos
    if env.explored_map[ox, oy] == 2:
        env.explored_map[ox, oy] = 1
    env.rover_pos = pos
    env.visit_counts[pos] = max(1, int(env.visit_counts[pos]))
    env.explored_map[pos] = 2


def save(name, env, cfg):
    with contextlib.redirect_stdout(io.StringIO()):
        frame = env.render()
    G, s = env.grid_size, env.cell_size
    assert frame.shape == (G * s, G * s, 3) and frame.dtype == np.uint8, (frame.shape, frame.dtype)
    scal = np.array([env.rover_pos[0], env.rover_pos[1], env.step_count, env.total_collisions,
                     int(env.collided_with_wall), int(env.completion_bonus_given), 0, 1], np.int32)
    np.savez_compressed(
        os.path.join(OUT, f"render_{name}.npz"), cfg=np.array(cfg, np.int32), cell_size=np.int32(s),
        cells=cells_of(env), visits=env.visit_counts.astype(np.int32), explored=env.explored_map.astype(np.int8),
        scalars=scal, frame=np.ascontiguousarray(frame))
    colours = len(np.unique(frame.reshape(-1, 3), axis=0))
    print(f"render_{name}: frame {frame.shape}, {colours} colours, rover {env.rover_pos}, "
          f"explored {int((env.explored_map > 0).sum())}/{G * G}", file=sys.stderr)


def rollout(env, rng, steps):
    for _ in range(steps):
        _, _, te, tr, _ = env.step(int(rng.integers(0, 5)))
        if te or tr:
            env.reset()


def gen_geometry(name, cfg, cell_size, seed):
    G, P, O, R, C = cfg
    rng = np.random.default_rng(seed)
    env = make(cfg, cell_size)
    with contextlib.redirect_stdout(io.StringIO()):
        random.seed(seed)
        env.reset()
        save(f"{name}_fresh", env, cfg)
        rollout(env, rng, 40)
        # both plant kinds in every later frame of the set
        kinds = list(env.plants.values())
        if all(kinds) or not any(kinds):
            first = next(iter(env.plants))
            env.plants[first] = not env.plants[first]
        save(f"{name}_rollout", env, cfg)
        move_rover(env, (0, 0))
        save(f"{name}_corner", env, cfg)
        move_rover(env, (G - 1, G // 2))
        save(f"{name}_edge", env, cfg)
        move_rover(env, (G - 1, G - 1))
        save(f"{name}_corner2", env, cfg)
        move_rover(env, list(env.plants)[-1])
        save(f"{name}_on_plant", env, cfg)
        beside = [(x + dx, y + dy) for (x, y) in sorted(env.obstacles) for dx, dy in ((0, 1), (1, 0), (0, -1), (-1, 0))
                  if 0 <= x + dx < G and 0 <= y + dy < G and (x + dx, y + dy) not in env.obstacles
                  and (x + dx, y + dy) not in env.plants]
        move_rover(env, beside[int(rng.integers(len(beside)))])
        save(f"{name}_beside_obstacle", env, cfg)
        seen = (rng.random((G, G)) < 0.9) & (cells_of(env) != OBST)
        env.explored_map[seen & (env.explored_map == 0)] = 1
        env.visit_counts[seen & (env.visit_counts == 0)] = 1
        rollout(env, rng, 10)
        save(f"{name}_explored", env, cfg)


def main():
    os.makedirs(OUT, exist_ok=True)
    for k, (name, (cfg, s)) in enumerate(GEOMETRIES.items()):
        gen_geometry(name, cfg, s, 100 + k)
    # one frame at the reference's own cell_size
    env = make(GEOMETRIES["g7"][0], 30)
    with contextlib.redirect_stdout(io.StringIO()):
        random.seed(3)
        env.reset()
        rollout(env, np.random.default_rng(3), 12)
    save("g7_s30", env, GEOMETRIES["g7"][0])


if __name__ == "__main__":
    main()
