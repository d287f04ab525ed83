"""The FIRST product of a kind (sixteen columns, one-triangle storage, transposed) must not be much slower than the later ones:
round 3 relocated / read the reduction segments with one blocking 64-byte copy per tile (some 30 000 at 1 M points: longer than
the build).  Reference entries: src/htool/hmatrix/hmatrix.hpp:113-138 (products), :64-78 (trans)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _clear_vram(gb=4.0):
    """The driver clears VRAM on its first use (~27 ms per GB) and what a process frees in the background (~45 ms per GB), and an
    allocation waits for that (NOTES.md).  The first 16-wide product allocates its ~1 GB workspace: pass `gb` GB through the
    driver and wait for its wipe, so that the allocation finds cleared memory whatever the box or the earlier tests left."""
    import torch

    a = torch.empty(int(gb * 1e9), dtype=torch.uint8, device="cuda")
    a.zero_()
    torch.cuda.synchronize()
    del a
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    time.sleep(1.0 + 0.06 * gb)


@pytest.mark.parametrize("sym", ["N", "S", "N+T"])
def test_first_wide_and_transposed_products_of_a_million_point_operator(built, sym):
    import torch

    import Htool
    from htool_python_amd.workloads import points_in_sphere
    from tests.helpers import cluster_of

    n = 1_000_000
    pts = points_in_sphere(n, seed=0)
    cl = cluster_of(pts, 100)
    at_build = sym == "N+T"  # the tables of the transposed product laid out by the build (HMatrixTreeBuilder.set_transposed_products)
    sym = sym[0]
    builder = Htool.HMatrixTreeBuilder(1e-3, 10.0, sym, "L" if sym == "S" else "N")
    if at_build:
        builder.set_transposed_products(True)
    H = builder.build(Htool.NativeGenerator("laplace", pts, pts), cl, cl)
    assert H.is_one_triangle() == (sym == "S")
    X = torch.rand(16, n, dtype=torch.float64, device="cuda")  # 16 columns, column stride n
    Y = torch.empty_like(X)
    st = torch.cuda.current_stream().cuda_stream
    t1 = _timed(lambda: H.matvec_device(X.data_ptr(), Y.data_ptr(), 0, st))
    t1b = _timed(lambda: H.matvec_device(X.data_ptr(), Y.data_ptr(), 0, st))
    y_one = Y[0].clone()
    _clear_vram()
    first = _timed(lambda: H.matmat_device(X.data_ptr(), n, Y.data_ptr(), n, 16, 0, st))
    second = _timed(lambda: H.matmat_device(X.data_ptr(), n, Y.data_ptr(), n, 16, 0, st))
    print("sym %s: one column %.1f / %.1f ms; 16 columns first %.1f ms, second %.1f ms" % (sym, 1e3 * t1, 1e3 * t1b, 1e3 * first, 1e3 * second))
    assert first - second < 0.020, (first, second)
    assert (Y[0] - y_one).norm().item() <= 1e-12 * y_one.norm().item()
    tr_first = _timed(lambda: H.matmat_device_trans("T", X.data_ptr(), n, Y.data_ptr(), n, 16, 0, st))
    tr_second = _timed(lambda: H.matmat_device_trans("T", X.data_ptr(), n, Y.data_ptr(), n, 16, 0, st))
    print("sym %s: transposed 16 columns first %.1f ms, second %.1f ms" % (sym, 1e3 * tr_first, 1e3 * tr_second))
    # (a general operator makes the index tables of the transposed product on first use -- DESIGN section 7, item 6 -- unless the
    # build was asked to lay them out: then the first transposed product only sets up its 16-wide workspace)
    assert tr_first - tr_second < (0.020 if (sym == "S" or at_build) else 0.8), (tr_first, tr_second)
    if at_build:  # the adjoint identity on the operator whose tables came with the build
        w = torch.rand(n, dtype=torch.float64, device="cuda")
        z = torch.empty_like(w)
        H.matmat_device_trans("T", w.data_ptr(), n, z.data_ptr(), n, 1, 0, st)
        H.matvec_device(X[1].contiguous().data_ptr(), Y[1].data_ptr(), 0, st)
        torch.cuda.synchronize()
        lhs, rhs = torch.dot(w, Y[1]).item(), torch.dot(z, X[1]).item()
        assert abs(lhs - rhs) < 1e-10 * abs(lhs)
    del H
    Htool.release_workspace()
