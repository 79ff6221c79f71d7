"""-m gpu: the mesh extraction under tests/poison.py's three fill bytes (0x00, 0xFF, 0x7F): no result may depend on what the extract
workspace and the outputs hold on entry, and no guard band may change. The extract workspace (edge masks, vertex bases, block
totals, the two counts) and the three outputs are torch.empty allocations of c3dgs_amd/mesh.py; the integration has no scratch of
its own (its planes are zeroed by contract), so it is run under each byte with whatever its callers allocate poisoned. Every
output is bit-equal across the three runs, and the 0xFF run is checked against tests/mesh_ref.py, so that being equal to a wrong
baseline is not enough."""
import numpy as np
import pytest
import torch

from tests import mesh_ref as mr, poison
from tests.test_mesh_gpu import (ORIGIN, H_VOX, assert_mesh, assert_planes, gpu_extract, gpu_integrate, new_volume, ref_integrate,
                                 zero_planes)

pytestmark = pytest.mark.gpu


def test_extract_workspace_and_outputs(hip):
    tsdf, weight, colors, origin, h = mr.random_lattice((37, 23, 11), seed=8)          # 9,361 points: 37 blocks, the last ragged
    ref = mr.extract(tsdf, weight, origin, h, colors)
    assert len(ref[2]) > 100

    def run():
        v, c, f = gpu_extract(tsdf, weight, origin, h, colors)
        return dict(vertices=v, colors=c, faces=f)

    poison.assert_independent(run, exact=("vertices", "colors", "faces"), check_bytes=(0xFF,),
                              check=lambda o: assert_mesh((o["vertices"], o["colors"], o["faces"]), ref, "poisoned extract"))


def test_integrate_then_extract(hip):
    """the fused sphere, colours included: planes and mesh under each byte"""
    ref = ref_integrate(zero_planes(True), "six", True)
    ref_mesh = mr.extract(ref[0], ref[1], ORIGIN, H_VOX, ref[2])
    assert len(ref_mesh[2]) > 100

    def run():
        vol = gpu_integrate(new_volume(True), "six", True)
        v, c, f = vol.extract()
        return dict(tsdf=vol.tsdf, weight=vol.weight, color=vol.color, vertices=v, colors=c, faces=f)

    def check(o):
        class Planes:
            tsdf, weight, color = (torch.from_numpy(o[k]) for k in ("tsdf", "weight", "color"))
        assert_planes(Planes, ref, "poisoned integrate")
        assert_mesh((o["vertices"], o["colors"], o["faces"]), ref_mesh, "poisoned integrate + extract")

    poison.assert_independent(run, exact=("tsdf", "weight", "color", "vertices", "colors", "faces"), check_bytes=(0xFF,), check=check)


def test_integrate_alone(hip):
    """no uninitialised allocation of its own: still the restatement's bits with the package's caches set aside under each byte"""
    ref = ref_integrate(zero_planes(False), "nineteen", False)
    poison.under_every_byte(lambda: assert_planes(gpu_integrate(new_volume(False), "nineteen", False), ref, "poisoned integrate"),
                            expect_allocations=False)
