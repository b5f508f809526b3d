"""What every stream-taking C entry checks on the host, before any device call, without a GPU: device_id < 0 is refused first
("no CPU path"), and the segmented entries refuse malformed host offsets with MMF_E_INVALID even when device_id names a
device that is not there."""
import ctypes

NO_DEVICE_ARGUMENT = {"mmf_version", "mmf_last_error", "mmf_padded_dim", "mmf_fast_scan_supported", "mmf_debug_query_order",
                      "mmf_debug_symmetric_schedule", "mmf_release_workspaces"}


def _lib():
    import multimodal_fusion_amd as mmf
    return mmf._lib, mmf._lib.lib()


def _zero(t):
    if issubclass(t, (ctypes.c_int, ctypes.c_int64)):
        return 0
    if issubclass(t, (ctypes.c_float, ctypes.c_double)):
        return 0.0
    return None


def test_every_entry_refuses_a_negative_device_first():
    m, L = _lib()
    visited = 0
    for name in m.EXPORTS + m.EXPORTS_COHORT:
        if name in NO_DEVICE_ARGUMENT:
            continue
        fn = getattr(L, name)
        assert tuple(fn.argtypes[-2:]) == (ctypes.c_int, ctypes.c_void_p), name
        args = [_zero(t) for t in fn.argtypes]
        args[-2] = -1
        assert fn(*args) == m.MMF_E_UNSUPPORTED, (name, L.mmf_last_error())
        assert b"no CPU path" in L.mmf_last_error(), (name, L.mmf_last_error())
        visited += 1
    assert visited == 35


def _segmented_calls():
    """name -> (call(ptr, n_seg), takes a row count of its own).  n = m = 4; host buffers stand in for device pointers."""
    m, L = _lib()
    buf = (ctypes.c_int64 * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    return L, m, {
        "mmf_simtopk_segmented": (lambda p, S: L.mmf_simtopk_segmented(b, 4, None, 4, 4, m.F32, m.COSINE, 1.0, 1, 0, p, None, S, b, b,
                                                                        None, None, 0, None), True),
        "mmf_kmeans_fit_segmented": (lambda p, S: L.mmf_kmeans_fit_segmented(b, 4, 4, p, S, 1, 1, 1, b, None, 1, 0.0, b, b, b, b, 0, None),
                                     True),
        "mmf_sim_dense_combined_segmented": (lambda p, S: L.mmf_sim_dense_combined_segmented(b, b, 4, 4, 1, p, S, 1.0, 1.0, b, 0, None),
                                             True),
        "mmf_offdiag_lower_median_segmented": (lambda p, S: L.mmf_offdiag_lower_median_segmented(b, p, S, b, 0, None), False),
        "mmf_threshold_edges_segmented_count": (lambda p, S: L.mmf_threshold_edges_segmented_count(b, p, S, b, b, b, 0, None), False),
        "mmf_threshold_edges_segmented_fill": (lambda p, S: L.mmf_threshold_edges_segmented_fill(b, p, S, b, b, b, b, 1, 0, None), False),
        "mmf_knn_clique_edges_count": (lambda p, S: L.mmf_knn_clique_edges_count(b, 4, 1, None, 0, p, S, b, b, b, 0, None), True),
        "mmf_knn_clique_edges_fill": (lambda p, S: L.mmf_knn_clique_edges_fill(b, 4, 1, None, 0, p, S, b, b, 1, 0, None), True),
        "mmf_lower_median_segmented": (lambda p, S: L.mmf_lower_median_segmented(b, p, S, b, 0, None), False),
    }


def test_segmented_entries_refuse_bad_offsets_before_any_device_call():
    L, m, calls = _segmented_calls()
    assert len(calls) == 9
    late, decreasing, short = (ctypes.c_int64 * 3)(1, 2, 4), (ctypes.c_int64 * 4)(0, 3, 2, 4), (ctypes.c_int64 * 3)(0, 2, 3)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)   # noqa: E731
    for name, (call, has_rows) in calls.items():
        assert call(vp(late), 2) == m.MMF_E_INVALID, (name, "start", L.mmf_last_error())
        assert call(vp(decreasing), 3) == m.MMF_E_INVALID, (name, "decreasing", L.mmf_last_error())
        assert b"segment 1" in L.mmf_last_error(), (name, L.mmf_last_error())
        if has_rows:      # the others read their row count from ptr: (0, 2, 3) is a valid table for them
            assert call(vp(short), 2) == m.MMF_E_INVALID, (name, "end", L.mmf_last_error())
