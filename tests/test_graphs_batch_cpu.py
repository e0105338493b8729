"""CPU: the host side of the batched graph build (fastegnn_radius_graph_batch_*, fastegnn_cutoff_edges_batch): workspace sizes
and the argument checks that run before any device call.  No compute calls (no GPU here)."""
import ctypes as C

import pytest
import torch

from fastegnn_amd import _lib as K

SOME = C.c_void_p(4096)   # a non-null pointer that no check may dereference


def test_batch_workspace_is_smaller_than_the_single_cloud_one():
    """The single-cloud workspace carries a start table over 2^24 cells; the batched one grows with N and B only."""
    L = K.lib()
    for N in (0, 1, 2, 77, 1000, 8000, 33333, 100000):
        for B in (0, 1, 2, 15, 500, 1000):
            assert L.fastegnn_radius_graph_batch_ws_bytes(N, B) < L.fastegnn_radius_graph_ws_bytes(N), (N, B)
    assert L.fastegnn_radius_graph_batch_ws_bytes(100000, 1000) < 16 << 20   # a quarter of the 64 MB start table alone


def test_workspace_sizes_do_not_decrease_in_any_argument():
    L = K.lib()
    Ns, Bs = (0, 1, 63, 64, 65, 1000, 100000, 1 << 22), (0, 1, 2, 9, 256, 257, 1000, 1 << 16)
    ws = [[L.fastegnn_radius_graph_batch_ws_bytes(N, B) for B in Bs] for N in Ns]
    for i in range(len(Ns)):
        for j in range(len(Bs)):
            assert ws[i][j] > 0
            assert i == 0 or ws[i][j] >= ws[i - 1][j]
            assert j == 0 or ws[i][j] >= ws[i][j - 1]
    Es = (0, 1, 63, 64, 65, 14252, 1 << 20, (1 << 31) - 1)
    tmp = [[L.fastegnn_cutoff_batch_tmp_bytes(E, B) for B in Bs] for E in Es]
    for i in range(len(Es)):
        for j in range(len(Bs)):
            assert tmp[i][j] > 0
            assert i == 0 or tmp[i][j] >= tmp[i - 1][j]
            assert j == 0 or tmp[i][j] >= tmp[i][j - 1]


def test_count_refuses_bad_arguments_before_any_device_call():
    L = K.lib()
    host = (C.c_int64 * 4)()
    big = L.fastegnn_radius_graph_batch_ws_bytes(10, 3)
    call = L.fastegnn_radius_graph_batch_count
    for args, msg in [((SOME, SOME, -1, 3, 0.1, SOME, big, host, None), b"N < 0"),
                      ((SOME, SOME, 10, -1, 0.1, SOME, big, host, None), b"B < 0"),
                      ((SOME, SOME, 10, 3, 0.0, SOME, big, host, None), b"r must be positive"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big, None, None), b"null edge_ptr_host"),
                      ((None, SOME, 10, 3, 0.1, SOME, big, host, None), b"null pointer"),
                      ((SOME, None, 10, 3, 0.1, SOME, big, host, None), b"null pointer"),
                      ((SOME, SOME, 10, 3, 0.1, None, big, host, None), b"null pointer"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big - 1, host, None), b"workspace too small")]:
        assert call(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"radius_graph_batch_count" in L.fastegnn_last_error()


def test_fill_refuses_bad_arguments_before_any_device_call():
    L = K.lib()
    big = L.fastegnn_radius_graph_batch_ws_bytes(10, 3)
    call = L.fastegnn_radius_graph_batch_fill
    for args, msg in [((SOME, SOME, -1, 3, 0.1, SOME, big, 5, SOME, SOME, SOME, None), b"N < 0"),
                      ((SOME, SOME, 10, -1, 0.1, SOME, big, 5, SOME, SOME, SOME, None), b"B < 0"),
                      ((SOME, SOME, 10, 3, -1.0, SOME, big, 5, SOME, SOME, SOME, None), b"r must be positive"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big, -1, SOME, SOME, SOME, None), b"n_edges out of range"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big, 1 << 31, SOME, SOME, SOME, None), b"n_edges out of range"),
                      ((SOME, SOME, 0, 3, 0.1, SOME, big, 5, SOME, SOME, None, None), b"edges without nodes"),
                      ((None, SOME, 10, 3, 0.1, SOME, big, 5, SOME, SOME, SOME, None), b"null pointer"),
                      ((SOME, None, 10, 3, 0.1, SOME, big, 5, SOME, SOME, SOME, None), b"null pointer"),
                      ((SOME, SOME, 10, 3, 0.1, None, big, 5, SOME, SOME, SOME, None), b"null pointer"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big, 5, None, SOME, SOME, None), b"null pointer"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big, 5, SOME, None, SOME, None), b"null pointer"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big, 5, SOME, SOME, None, None), b"null pointer"),
                      ((SOME, SOME, 10, 3, 0.1, SOME, big - 1, 5, SOME, SOME, SOME, None), b"workspace too small")]:
        assert call(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"radius_graph_batch_fill" in L.fastegnn_last_error()


def test_cutoff_refuses_bad_arguments_before_any_device_call():
    L = K.lib()
    big = L.fastegnn_cutoff_batch_tmp_bytes(100, 3)
    call = L.fastegnn_cutoff_edges_batch
    for args, msg in [((SOME, SOME, SOME, SOME, -1, 100, 50, SOME, SOME, SOME, big, None), b"B < 0"),
                      ((SOME, SOME, SOME, SOME, 3, -1, 0, SOME, SOME, SOME, big, None), b"E out of range"),
                      ((SOME, SOME, SOME, SOME, 3, 1 << 31, 50, SOME, SOME, SOME, big, None), b"E out of range"),
                      ((SOME, SOME, SOME, SOME, 3, 100, 101, SOME, SOME, SOME, big, None), b"keep_total out of range"),
                      ((SOME, SOME, SOME, SOME, 3, 100, -1, SOME, SOME, SOME, big, None), b"keep_total out of range"),
                      ((None, SOME, SOME, SOME, 3, 100, 50, SOME, SOME, SOME, big, None), b"null pointer"),
                      ((SOME, None, SOME, SOME, 3, 100, 50, SOME, SOME, SOME, big, None), b"null pointer"),
                      ((SOME, SOME, None, SOME, 3, 100, 50, SOME, SOME, SOME, big, None), b"null pointer"),
                      ((SOME, SOME, SOME, None, 3, 100, 50, SOME, SOME, SOME, big, None), b"null pointer"),
                      ((SOME, SOME, SOME, SOME, 3, 100, 50, None, SOME, SOME, big, None), b"null pointer"),
                      ((SOME, SOME, SOME, SOME, 3, 100, 50, SOME, SOME, None, big, None), b"null pointer"),
                      ((SOME, SOME, SOME, SOME, 3, 100, 50, SOME, SOME, SOME, big - 1, None), b"tmp too small")]:
        assert call(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"cutoff_edges_batch" in L.fastegnn_last_error()


def test_no_nodes_or_no_graphs_is_ok_with_zero_counts():
    L = K.lib()
    for N, B in [(0, 0), (0, 3), (10, 0)]:
        host = (C.c_int64 * (B + 1))(*([7] * (B + 1)))
        assert L.fastegnn_radius_graph_batch_count(None, None, N, B, 0.1, None, 0, host, None) == 0
        assert list(host) == [0] * (B + 1)
        assert L.fastegnn_radius_graph_batch_fill(None, None, N, B, 0.1, None, 0, 0, None, None, None, None) == 0
    assert L.fastegnn_cutoff_edges_batch(None, None, None, None, 0, 0, 0, None, None, None, 0, None) == 0
    assert L.fastegnn_cutoff_edges_batch(None, None, None, None, 3, 100, 0, None, None, None, 0, None) == 0


def test_python_entry_points_refuse_cpu_tensors():
    from fastegnn_amd.graphs import cutoff_edges_batch, radius_graph_batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        radius_graph_batch(torch.rand(10, 3), [0, 4, 10], 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cutoff_edges_batch(torch.zeros(2, 4, dtype=torch.int64), torch.rand(4), [0, 2, 4], 0.5)
