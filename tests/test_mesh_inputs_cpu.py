"""The input layer of the mesh stages (humanliff_amd/NeRF/mesh.py) without a device: one table of bad meshes through every public entry
that takes a mesh, against what each entry did before the stages shared the layer, and the layer's own grid and index rules."""
import numpy as np
import pytest
import torch

from humanliff_amd.NeRF import distance, mesh, raster, simplify

N, T = 5, 2
V = np.arange(15, dtype=np.float64).reshape(N, 3) * 0.01
TRI = np.array([[0, 1, 2], [2, 3, 4]])
NRM = np.ones((N, 3))
GOOD = (V, TRI)
I3, Z3 = np.eye(3), np.zeros(3)

# case -> (mesh dict or vertices, `triangles`, `normals` argument or None)
CASES = {
    "vertices (N,2)": (V[:, :2], TRI, None),
    "integer vertices": (V.astype(np.int64), TRI, None),
    "triangles (T,2)": (V, TRI[:, :2], None),
    "float triangles": (V, TRI.astype(np.float32), None),
    "zero triangles": (V, TRI[:0], None),
    "dict plus triangles": ({"vertices": V, "triangles": TRI}, TRI, None),
    "vertices without triangles": (V, None, None),
    "CPU tensor vertices": (torch.zeros(N, 3), TRI, None),
    "CPU tensor triangles": (V, torch.zeros(T, 3, dtype=torch.int64), None),
    "CPU tensor normals argument": (V, TRI, torch.ones(N, 3)),
    "CPU tensor normals in the dict": ({"vertices": V, "triangles": TRI, "normals": torch.ones(N, 3)}, None, None),
}


def _pair(m, t):
    return m if isinstance(m, dict) else (m, t)


# entry -> call(mesh, triangles, normals).  An entry without a `normals` argument ignores the third.
ENTRIES = {
    "simplify_mesh": lambda m, t, n: simplify.simplify_mesh(m, t, cell=0.02, normals=n),
    "point_mesh_distance": lambda m, t, n: distance.point_mesh_distance(V, m, t, normals=n),
    "build_index": lambda m, t, n: distance.build_index(m, t),
    "sample_surface": lambda m, t, n: distance.sample_surface(m, 16, t),
    "mesh_distance": lambda m, t, n: distance.mesh_distance(_pair(m, t), GOOD),
    "rasterize": lambda m, t, n: raster.rasterize(m, t, 4, 6, I3, I3, Z3, normals=n),
}
NO_NORMALS_ARGUMENT = ("build_index", "sample_surface", "mesh_distance")
NO_TRIANGLES_ARGUMENT = ("mesh_distance",)              # (it takes dicts or pairs: a dict beside `triangles` cannot be written)

# What every (entry, case) raised before the stages shared mesh.py, recorded by running this table on that commit: the exception type
# and the argument its message names.  DEVICE: accepted by the host checks - with no device the entry gets as far as asking for one.
DEVICE = (RuntimeError, "needs")
V_, T_, N_ = (ValueError, "vertices"), (ValueError, "triangles"), (RuntimeError, "normals")
CPU_V, CPU_T = (RuntimeError, "vertices"), (RuntimeError, "triangles")
COMMON = {"vertices (N,2)": V_, "integer vertices": V_, "triangles (T,2)": T_, "float triangles": T_, "zero triangles": T_,
          "dict plus triangles": T_, "vertices without triangles": T_, "CPU tensor vertices": CPU_V, "CPU tensor triangles": CPU_T}
EXPECT = {(entry, case): kind for entry in ENTRIES for case, kind in COMMON.items()}
EXPECT.update({
    ("simplify_mesh", "CPU tensor normals argument"): N_,
    ("simplify_mesh", "CPU tensor normals in the dict"): N_,                    # the simplifier uses a dict's normals
    ("point_mesh_distance", "CPU tensor normals argument"): N_,
    ("point_mesh_distance", "CPU tensor normals in the dict"): DEVICE,          # the target's normals play no part
    ("build_index", "CPU tensor normals in the dict"): DEVICE,
    ("sample_surface", "CPU tensor normals in the dict"): DEVICE,
    ("mesh_distance", "CPU tensor normals in the dict"): DEVICE,                # (refused once there is a device to ask for)
    ("rasterize", "integer vertices"): DEVICE,                                  # rasterize converts vertices of any dtype
    ("rasterize", "dict plus triangles"): V_,                                   # rasterize takes arrays only: a dict is no (N,3)
    ("rasterize", "CPU tensor normals argument"): N_,
    ("rasterize", "CPU tensor normals in the dict"): T_,                        # (arrays only: `triangles` is what is missing)
})
del EXPECT["mesh_distance", "dict plus triangles"]


def outcome(entry, case):
    """-> (exception type, message) of ENTRIES[entry] on CASES[case]."""
    try:
        ENTRIES[entry](*CASES[case])
    except Exception as e:  # noqa: BLE001
        return type(e), str(e)
    return None, ""


def applicable(entry, case):
    return not (case == "CPU tensor normals argument" and entry in NO_NORMALS_ARGUMENT or
                case == "dict plus triangles" and entry in NO_TRIANGLES_ARGUMENT)


@pytest.fixture()
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_bad_meshes_are_refused_as_before(entry, no_device):
    for case in CASES:
        if not applicable(entry, case):
            assert (entry, case) not in EXPECT
            continue
        kind, word = EXPECT[entry, case]
        got, message = outcome(entry, case)
        print(f"{entry}: {case}: {None if got is None else got.__name__}: {message}")
        assert got is kind and word in message, (entry, case, message)


def test_grid_extents():
    """(origin, g) as simplify.grid_extents gave them before it moved: g = floor((hi - origin) / cell) + 1."""
    lo, hi, cell = np.array([0.0, -1.0, 2.0]), np.array([1.0, 1.0, 2.5]), np.array([0.25, 0.5, 1.0])
    o, g = mesh.grid_extents(lo, hi, cell, None, 1 << 31, "t")
    assert np.array_equal(o, lo) and o is not lo and g.dtype == np.int64 and g.tolist() == [5, 5, 1]
    org = np.array([-0.1, -1.0, 0.0])
    o, g = mesh.grid_extents(lo, hi, cell, org, 1 << 31, "t")
    assert o is org and g.tolist() == [5, 5, 3]                          # floor(1.1 / 0.25) = 4, floor(2 / 0.5) = 4, floor(2.5) = 2
    o, g = mesh.grid_extents(lo, lo, cell, None, 1 << 27, "t")           # hi == lo: one cell
    assert np.array_equal(o, lo) and g.tolist() == [1, 1, 1]
    one = np.ones(3)
    for cap, bits in ((1 << 31, 31), (1 << 27, 27)):
        side = np.array([1 << (bits - 20), 1 << 10, 1 << 10], dtype=np.float64)
        assert mesh.grid_extents(Z3, side - 1.0, one, None, cap, "t")[1].tolist() == side.tolist()           # exactly the cap
        with pytest.raises(ValueError, match=rf"t: .*2\^{bits}"):
            mesh.grid_extents(Z3, side - 1.0 + np.array([0.0, 0.0, 1.0]), one, None, cap, "t")              # one layer more
        with pytest.raises(ValueError, match=rf"t: .*2\^{bits}"):
            mesh.grid_extents(Z3, np.array([float(cap), 0.0, 0.0]), one, None, cap, "t")                    # one axis alone
    with pytest.raises(ValueError, match=r"2\^31"):
        mesh.grid_extents(Z3, np.array([np.inf, 0.0, 0.0]), one, None, 1 << 31, "t")


def test_device_triangles_rule_on_the_host():
    """An index that does not fit int32 becomes -1; int32 passes through untouched; any integer dtype is taken."""
    big = np.array([[0, 1, 2], [-1, 1 << 31, (1 << 31) - 1], [1 << 40, -(1 << 40), 3]], dtype=np.int64)
    got = mesh.device_triangles(big, "cpu")
    assert got.dtype == torch.int32 and got.is_contiguous()
    assert got.tolist() == [[0, 1, 2], [-1, -1, (1 << 31) - 1], [-1, -1, 3]]
    assert mesh.device_triangles(torch.from_numpy(big), "cpu").tolist() == got.tolist()
    i32 = torch.tensor([[0, -5, 7]], dtype=torch.int32)
    assert mesh.device_triangles(i32, "cpu").data_ptr() == i32.data_ptr()                                   # untouched, -5 included
    assert mesh.device_triangles(np.array([[0, 65535, 7]], dtype=np.uint16), "cpu").tolist() == [[0, 65535, 7]]
    assert raster.device_triangles is mesh.device_triangles
    f = mesh.to_device(np.arange(6, dtype=np.float32).reshape(2, 3)[:, ::-1], torch.float64, "cpu")
    assert f.dtype == torch.float64 and f.is_contiguous() and f.tolist() == [[2.0, 1.0, 0.0], [5.0, 4.0, 3.0]]
