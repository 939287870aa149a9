"""The geometries of the policy / rollout / replay parity tests beyond g20 and g21 (test infra):
obs lengths chosen by residue -- what the staging pitch D | 1, the K padding to 8, the hidden
buffers' rows and the replay kernels' dword paths do with them -- and by the step kernel that
writes their obs.

    id       D    what it exercises                                        step kernel
    e52      52   D even: pitch 53 != D; D % 8 = 4; D % 4 = 0              pe_step_quad<runtime C,R,1word,bytetile>
    e72      72   Kp0 == D: no padded k-group; pitch 73                    pe_step_quad<runtime C,R,1word,bytetile>
    p57      57   7 padded columns; D % 4 = 1                              pe_step_quad<runtime C,R,1word[,bytetile]>
    p87      87   1 padded column                                          pe_step_quad<runtime C,R,1word>
    w347     347  byte-tile codes; HB = pitch; only 32-env tiles fit       pe_step_quad<C64,R6,bytetile>
    far347   347  far kernel's codes, the R = 32 code table                pe_step_far<C64,R32,bytetile>
    max417   417  the longest obs a [[32, 5]] net's LDS images hold        pe_step_wave
    over422  422  one lidar channel more: refused                          pe_step_wave

The kernel names are what pe_internal_plan gives (asserted without a device in
test_policy_geometries_host.py, and on the device by `make`).  Every row of the table was
accepted as stated: none had to be swapped for a neighbour.
"""
DEV = "cuda:0"

# cfg: (grid, plants, obstacles, range, channels); obs: the forms the batch is fed to a policy in
GEO = {
    "e52": dict(cfg=(8, 3, 3, 4, 5), obs=("codes",)),
    "e72": dict(cfg=(10, 4, 4, 5, 9), obs=("codes",)),
    "p57": dict(cfg=(9, 3, 3, 3, 6), obs=("codes", "f32")),
    "p87": dict(cfg=(12, 4, 6, 7, 12), obs=("f32",)),
    "w347": dict(cfg=(24, 10, 12, 6, 64), obs=("codes",)),
    "far347": dict(cfg=(33, 12, 20, 32, 64), obs=("codes",)),
    "max417": dict(cfg=(12, 4, 6, 3, 78), obs=("f32",)),
    "over422": dict(cfg=(12, 4, 6, 3, 79), obs=("f32",)),
}
KERNEL = {
    ("e52", True): "pe_step_quad<runtime C,R,1word,bytetile>",
    ("e72", True): "pe_step_quad<runtime C,R,1word,bytetile>",
    ("p57", True): "pe_step_quad<runtime C,R,1word,bytetile>",
    ("p57", False): "pe_step_quad<runtime C,R,1word>",
    ("p87", False): "pe_step_quad<runtime C,R,1word>",
    ("w347", True): "pe_step_quad<C64,R6,bytetile>",
    ("far347", True): "pe_step_far<C64,R32,bytetile>",
    ("max417", False): "pe_step_wave",
    ("over422", False): "pe_step_wave",
}


def obs_dim(name):
    return 5 * GEO[name]["cfg"][4] + 27


def replay_geometry(name):
    """(grid_size, lidar_range, lidar_channels), as pe_replay_store and replay_util take it"""
    G, _, _, R, C = GEO[name]["cfg"]
    return G, R, C


def make(name, n, codes, **kw):
    """A PlantOSBatch of geometry `name` on the device; asserts the step kernel of the table."""
    from plantos_amd import PlantOSBatch
    G, P, Ob, R, C = GEO[name]["cfg"]
    b = PlantOSBatch(n, grid_size=G, num_plants=P, num_obstacles=Ob, lidar_range=R, lidar_channels=C,
                     device=DEV, obs_codes=codes, **kw)
    assert b.kernel_name == KERNEL[(name, codes)], (name, codes, b.kernel_name)
    assert b.obs_dim == obs_dim(name)
    return b
