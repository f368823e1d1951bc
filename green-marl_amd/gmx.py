"""ctypes binding of libgmx.so -- the Python host-side mirror of the C ABI in include/gmx.h.

The product path.  There is NO CPU fallback here: if libgmx.so is missing or no
gfx950 device is visible, every compute entry raises.  (The CPU oracle lives in
oracle/ and is only ever loaded by tests / smoke / bench's cpu_baseline leg.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GMX_LIB") or os.path.join(_HERE, "libgmx.so")   # GMX_LIB: the debug build of a test

GMX_GRAPH_SORT_ROWS = 0x1
GMX_GRAPH_NO_REVERSE = 0x2
GMX_PR_RELABEL = 0x1
GMX_PR_HOT_LDS = 0x2
GMX_PR_SLICED = 0x4
GMX_PR_COLD_PB = 0x8
INT_MAX = 2147483647


class GmxError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("last_diff", C.c_double),
                ("kernel_ms", C.c_double), ("h2d_ms", C.c_double), ("d2h_ms", C.c_double),
                ("edges_examined", C.c_int64), ("vertices_reached", C.c_int64), ("edges_reached", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 32), ("compute_units", C.c_int32),
                ("clock_mhz", C.c_int32), ("hbm_bytes", C.c_int64), ("l2_bytes", C.c_int32),
                ("lds_bytes_per_cu", C.c_int32)]


class PrColdShape(C.Structure):   # gmx_pr_cold_shape_t
    _fields_ = [("groups", C.c_int64 * 7), ("supersteps", C.c_uint32 * 7), ("items2_sole", C.c_int64),
                ("items2_chunk", C.c_int64), ("bins_few", C.c_int64), ("bins_many", C.c_int64),
                ("tiles_by_mode", C.c_int64 * 4), ("fused", C.c_int32)]


PR_COLD_FORMS = ("edge", "pair", "E1", "E2", "E4", "E8", "H")          # index order of groups / supersteps
PR_COLD_TILE_MODES = ("edge", "pair", "classed", "singles")            # index order of tiles_by_mode


EXPORTS = [
    "gmx_workspace_bytes", "gmx_workspace_release", "gmx_last_error", "gmx_device_count", "gmx_set_device", "gmx_device_info", "gmx_copy_bandwidth",
    "gmx_graph_upload", "gmx_graph_from_edges", "gmx_graph_create_rmat", "gmx_graph_free", "gmx_graph_symmetrize",
    "gmx_graph_num_nodes", "gmx_graph_num_edges", "gmx_graph_download", "gmx_graph_edge_order",
    "gmx_graph_upload_e64", "gmx_graph_download_e64", "gmx_graph_edge_order_e64", "gmx_graph_reverse_edge_map_e64",
    "gmx_pagerank_f64", "gmx_pagerank_f32", "gmx_hop_dist", "gmx_bfs_levels", "gmx_bc", "gmx_bc_batch", "gmx_bc_all", "gmx_sssp", "gmx_sssp_path", "gmx_sssp_path_f64", "gmx_route_create", "gmx_route_free", "gmx_route_query", "gmx_bidir_dijkstra", "gmx_scc", "gmx_wcc", "gmx_kcore", "gmx_msf", "gmx_coloring", "gmx_closeness", "gmx_communities", "gmx_avg_teen_cnt", "gmx_conduct", "gmx_triangle_counting", "gmx_triangle_counting_part", "gmx_triangle_counting_cn", "gmx_triangle_counting_directed", "gmx_triangle_counting_directed_part", "gmx_clustering", "gmx_biconnected", "gmx_ktruss", "gmx_kclique", "gmx_squares", "gmx_graphlets", "gmx_louvain", "gmx_common_nbrs", "gmx_common_nbr_counts", "gmx_adamic_adar", "gmx_v_cover", "gmx_random_bipartite_matching", "gmx_random_walk_sampling", "gmx_node_sampling", "gmx_potential_friends", "gmx_graph_reverse_edge_map",
    "gmx_bfs_create", "gmx_bfs_free", "gmx_bfs_start", "gmx_bfs_step_begin", "gmx_bfs_found_bitmap", "gmx_bfs_step_end",
    "gmx_bfs_download",
    "gmx_pr_create", "gmx_pr_free", "gmx_pr_reset", "gmx_pr_step", "gmx_pr_contrib_slice",
    "gmx_pr_contrib_full", "gmx_pr_exchange_count", "gmx_pr_diff_ptr", "gmx_pr_diff", "gmx_pr_download", "gmx_pr_work",
    "gmx_pr_set_chunks", "gmx_pr_num_chunks", "gmx_pr_chunk_range", "gmx_pr_step_chunk", "gmx_pr_contrib_next_full",
    "gmx_ipc_export", "gmx_ipc_open", "gmx_ipc_close", "gmx_pr_contrib_buffers", "gmx_pr_set_peers",
    "gmx_pr_push_chunk", "gmx_pr_push_current", "gmx_pr_push_join",
    "gmx_pr_packed_info", "gmx_pr_recv_buffers", "gmx_pr_set_peers_packed", "gmx_pr_push_packed", "gmx_pr_unpack", "gmx_pr_recv_list",
    "gmx_pr_gather_classes", "gmx_pr_step_gather", "gmx_pr_push_join_chunk", "gmx_pr_gather_items",
    "gmx_pr_timing", "gmx_pr_kernel_time", "gmx_pr_kernel_name", "gmx_pr_default_options", "gmx_pr_cold_info",
    "gmx_pr_cold_shape",
]

_LIB = None
IPC_HANDLE_BYTES = 64   # GMX_IPC_HANDLE_BYTES


def lib():
    """Load libgmx.so (raises if the HIP extension has not been built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GmxError("libgmx.so not built: run `make -C green-marl_amd lib` (or __graft_entry__.build())")
        # PyTorch-ROCm bundles its own HIP runtime (same soname as /opt/rocm's).  Whichever is loaded first
        # serves the whole process; torch must be that one, or its own device discovery fails later
        # ("No HIP GPUs are available") when the multi-GPU driver wraps these buffers in tensors.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        L.gmx_last_error.restype = C.c_char_p
        L.gmx_workspace_bytes.restype = C.c_int64
        L.gmx_device_count.argtypes = [C.POINTER(C.c_int)]
        L.gmx_set_device.argtypes = [C.c_int]
        L.gmx_device_info.argtypes = [C.POINTER(DeviceInfo)]
        L.gmx_copy_bandwidth.argtypes = [i64, C.c_int, C.POINTER(C.c_double)]
        L.gmx_graph_upload.argtypes = [vp, vp, vp, vp, i64, i64, C.c_uint32, C.POINTER(vp)]
        L.gmx_graph_from_edges.argtypes = [vp, vp, i64, i64, C.c_uint32, C.POINTER(vp)]
        L.gmx_graph_create_rmat.argtypes = [i64, i64, C.c_long, C.c_double, C.c_double, C.c_double, C.c_int,
                                            C.c_uint32, C.POINTER(vp)]
        L.gmx_graph_free.argtypes = [vp]
        L.gmx_graph_symmetrize.argtypes = [vp, C.POINTER(vp)]
        L.gmx_graph_num_nodes.argtypes = [vp]
        L.gmx_graph_num_nodes.restype = i64
        L.gmx_graph_num_edges.argtypes = [vp]
        L.gmx_graph_num_edges.restype = i64
        L.gmx_graph_download.argtypes = [vp, vp, vp, vp, vp]
        L.gmx_graph_edge_order.argtypes = [vp, vp, C.POINTER(C.c_int)]
        L.gmx_pagerank_f64.argtypes = [vp, C.c_double, C.c_double, i32, vp, C.POINTER(Stats)]
        L.gmx_pagerank_f32.argtypes = [vp, C.c_float, C.c_float, i32, vp, C.POINTER(Stats)]
        L.gmx_hop_dist.argtypes = [vp, i32, vp, C.POINTER(Stats)]
        L.gmx_common_nbrs.argtypes = [vp, i32, i32, vp, i64, C.POINTER(i64)]
        L.gmx_common_nbr_counts.argtypes = [vp, vp, vp, i64, vp]
        L.gmx_triangle_counting_cn.argtypes = [vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_adamic_adar.argtypes = [vp, vp, C.POINTER(Stats)]
        L.gmx_v_cover.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(Stats)]
        L.gmx_random_bipartite_matching.argtypes = [vp, vp, vp, C.POINTER(i32), C.POINTER(Stats)]
        L.gmx_random_walk_sampling.argtypes = [vp, C.c_float, C.c_float, i32, i32, C.POINTER(C.c_uint64), vp, vp, C.POINTER(i64), C.POINTER(i32),
                                               C.POINTER(Stats)]
        L.gmx_node_sampling.argtypes = [vp, C.c_int, i32, C.POINTER(C.c_uint64), vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_bfs_levels.argtypes = [vp, i32, vp, C.POINTER(i32)]
        L.gmx_bc.argtypes = [vp, vp, i32, C.c_int, vp, C.POINTER(Stats)]
        L.gmx_bc_batch.argtypes = [vp, vp, i32, C.c_int, i32, vp, C.POINTER(Stats)]
        L.gmx_bc_all.argtypes = [vp, C.c_int, i32, vp, C.POINTER(Stats)]
        L.gmx_triangle_counting.argtypes = [vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_sssp.argtypes = [vp, i32, vp, vp, C.POINTER(Stats)]
        L.gmx_sssp_path.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(Stats)]
        L.gmx_sssp_path_f64.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.POINTER(Stats)]
        L.gmx_route_create.argtypes = [vp, vp, C.POINTER(vp)]
        L.gmx_route_free.argtypes = [vp]
        L.gmx_route_query.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i64), vp, vp, i64, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_bidir_dijkstra.argtypes = [vp, vp, i32, i32, vp, vp, C.POINTER(i32), C.POINTER(Stats)]
        L.gmx_scc.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_wcc.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_kcore.argtypes = [vp, C.c_int, vp, vp, C.POINTER(i32), C.POINTER(Stats)]
        L.gmx_coloring.argtypes = [vp, vp, vp, vp, C.POINTER(i32), C.POINTER(Stats)]
        L.gmx_closeness.argtypes = [vp, C.c_int, vp, i32, vp, vp, vp, vp, C.POINTER(Stats)]
        L.gmx_msf.argtypes = [vp, vp, vp, C.POINTER(i64), C.POINTER(i64), vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_communities.argtypes = [vp, i32, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(Stats)]
        L.gmx_potential_friends.argtypes = [vp, i32, i32, vp, vp, i64, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_avg_teen_cnt.argtypes = [vp, vp, i32, vp, C.POINTER(C.c_float), C.POINTER(Stats)]
        L.gmx_conduct.argtypes = [vp, vp, i32, C.POINTER(C.c_float), C.POINTER(Stats)]
        L.gmx_graph_reverse_edge_map.argtypes = [vp, vp]
        L.gmx_graph_upload_e64.argtypes = [vp, vp, vp, vp, i64, i64, C.c_uint32, C.POINTER(vp)]
        L.gmx_graph_download_e64.argtypes = [vp, vp, vp, vp, vp]
        L.gmx_graph_edge_order_e64.argtypes = [vp, vp, C.POINTER(C.c_int)]
        L.gmx_graph_reverse_edge_map_e64.argtypes = [vp, vp]
        L.gmx_triangle_counting_part.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_triangle_counting_directed.argtypes = [vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_triangle_counting_directed_part.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_clustering.argtypes = [vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_biconnected.argtypes = [vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_ktruss.argtypes = [vp, vp, vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_kclique.argtypes = [vp, i32, vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_squares.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_graphlets.argtypes = [vp, C.c_int, vp, vp, C.POINTER(Stats)]
        L.gmx_louvain.argtypes = [vp, vp, i32, i32, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(Stats)]
        L.gmx_bfs_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.gmx_bfs_free.argtypes = [vp]
        L.gmx_bfs_start.argtypes = [vp, i32]
        L.gmx_bfs_step_begin.argtypes = [vp, C.POINTER(C.c_int)]
        L.gmx_bfs_found_bitmap.argtypes = [vp, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.gmx_bfs_step_end.argtypes = [vp, C.POINTER(i64)]
        L.gmx_bfs_download.argtypes = [vp, vp, C.POINTER(Stats)]
        L.gmx_pr_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(vp)]
        L.gmx_pr_free.argtypes = [vp]
        L.gmx_pr_reset.argtypes = [vp, C.c_double]
        L.gmx_pr_step.argtypes = [vp, vp]
        L.gmx_pr_contrib_slice.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
        L.gmx_pr_contrib_full.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
        L.gmx_pr_diff_ptr.argtypes = [vp, C.POINTER(vp)]
        L.gmx_ipc_export.argtypes = [vp, vp]
        L.gmx_ipc_open.argtypes = [vp, C.POINTER(vp)]
        L.gmx_ipc_close.argtypes = [vp]
        L.gmx_pr_contrib_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
        L.gmx_pr_set_peers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.gmx_pr_push_chunk.argtypes = [vp, C.c_int, vp]
        L.gmx_pr_push_current.argtypes = [vp, vp]
        L.gmx_pr_push_join.argtypes = [vp, vp]
        L.gmx_pr_gather_classes.argtypes = [vp, C.POINTER(C.c_int)]
        L.gmx_pr_step_gather.argtypes = [vp, C.c_int, vp]
        L.gmx_pr_gather_items.argtypes = [vp, C.c_int, C.POINTER(i64)]
        L.gmx_pr_push_join_chunk.argtypes = [vp, C.c_int, vp]
        L.gmx_pr_packed_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.gmx_pr_recv_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
        L.gmx_pr_set_peers_packed.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)]
        L.gmx_pr_push_packed.argtypes = [vp, C.c_int, vp]
        L.gmx_pr_unpack.argtypes = [vp, C.c_int, vp]
        L.gmx_pr_recv_list.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(i64)]
        L.gmx_pr_set_chunks.argtypes = [vp, C.c_int]
        L.gmx_pr_num_chunks.argtypes = [vp, C.POINTER(C.c_int)]
        L.gmx_pr_chunk_range.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(i64)]
        L.gmx_pr_step_chunk.argtypes = [vp, C.c_int, vp]
        L.gmx_pr_contrib_next_full.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
        L.gmx_pr_exchange_count.argtypes = [vp, C.POINTER(i64)]
        L.gmx_pr_diff.argtypes = [vp, vp, C.POINTER(C.c_double)]
        L.gmx_pr_download.argtypes = [vp, vp]
        L.gmx_pr_work.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.gmx_pr_cold_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.gmx_pr_cold_shape.argtypes = [vp, C.POINTER(PrColdShape)]
        L.gmx_pr_default_options.argtypes = [i64, C.c_int]
        L.gmx_pr_default_options.restype = C.c_uint32
        L.gmx_pr_timing.argtypes = [vp, C.c_int]
        L.gmx_pr_kernel_time.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double)]
        L.gmx_pr_kernel_name.argtypes = [vp]
        L.gmx_pr_kernel_name.restype = C.c_char_p
        _LIB = L
    return _LIB


def _ck(status):
    if status != 0:
        raise GmxError("gmx status %d: %s" % (status, lib().gmx_last_error().decode(errors="replace")))


def device_count():
    n = C.c_int(0)
    st = lib().gmx_device_count(C.byref(n))
    return n.value if st == 0 else 0


def require_device():
    if device_count() < 1:
        raise GmxError("no HIP device visible: the gmx hot path has no CPU fallback")


def set_device(i):
    _ck(lib().gmx_set_device(i))


def device_info():
    d = DeviceInfo()
    _ck(lib().gmx_device_info(C.byref(d)))
    return {"name": d.name.decode(), "arch": d.arch.decode(), "compute_units": d.compute_units,
            "clock_mhz": d.clock_mhz, "hbm_bytes": d.hbm_bytes, "l2_bytes": d.l2_bytes,
            "lds_bytes_per_cu": d.lds_bytes_per_cu}


def copy_bandwidth(nbytes=1 << 30, iters=10):
    """Measured device copy rate in GB/s (bytes read + written)."""
    g = C.c_double(0)
    _ck(lib().gmx_copy_bandwidth(nbytes, iters, C.byref(g)))
    return g.value


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


class Route:
    """gmx_route_t: the weights of Graph.route() on the device and the scratch of a query."""

    def __init__(self, graph, handle):
        self._g = graph          # borrowed: keeps the graph alive as long as the route
        self._h = handle

    def query(self, src, dst, cap=None):
        """One pair -> (found, cost or None, path_node[int32], path_edge[int32], hops, stats): the vertices after src up to dst
        and the uploaded forward slot of the edge into each; with cap < hops the first cap of them."""
        if not self._h:
            raise GmxError("route has been freed")
        cap = self._g.V if cap is None else int(cap)
        pn, pe = (np.zeros(max(cap, 1), np.int32) for _ in range(2))
        found, cost, hops, st = C.c_int32(0), C.c_int64(0), C.c_int64(0), Stats()
        _ck(lib().gmx_route_query(self._h, int(src), int(dst), C.byref(found), C.byref(cost), pn.ctypes.data, pe.ctypes.data, cap,
                                  C.byref(hops), C.byref(st)))
        k = min(hops.value, cap)
        return bool(found.value), (cost.value if found.value else None), pn[:k], pe[:k], hops.value, st.as_dict()

    def free(self):
        if self._h:
            lib().gmx_route_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Graph:
    """Device-resident CSR (+ reverse CSR) in gm_graph's layout."""

    def __init__(self, handle):
        self._h = handle

    # -- constructors ------------------------------------------------------
    @classmethod
    def upload(cls, begin, node_idx, r_begin=None, r_node_idx=None, flags=0):
        require_device()
        begin, node_idx = _i32(begin), _i32(node_idx)
        V, E = len(begin) - 1, len(node_idx)
        h = C.c_void_p()
        rb = _i32(r_begin) if r_begin is not None else None
        rn = _i32(r_node_idx) if r_node_idx is not None else None
        _ck(lib().gmx_graph_upload(begin.ctypes.data, node_idx.ctypes.data if E else None,
                                   rb.ctypes.data if rb is not None else None,
                                   rn.ctypes.data if (rn is not None and E) else None,
                                   V, E, flags, C.byref(h)))
        return cls(h)

    @classmethod
    def from_edges(cls, V, src, dst, flags=0):
        require_device()
        src, dst = _i32(src), _i32(dst)
        h = C.c_void_p()
        E = len(src)
        _ck(lib().gmx_graph_from_edges(src.ctypes.data if E else None, dst.ctypes.data if E else None,
                                       V, E, flags, C.byref(h)))
        return cls(h)

    @classmethod
    def rmat(cls, N, M, seed=1997, a=0.57, b=0.19, c=0.19, permute=False, flags=0):
        require_device()
        h = C.c_void_p()
        _ck(lib().gmx_graph_create_rmat(N, M, seed, a, b, c, int(permute), flags, C.byref(h)))
        return cls(h)

    def symmetrize(self):
        """Undirected simple version (both orientations, duplicates and self loops dropped)."""
        h = C.c_void_p()
        _ck(lib().gmx_graph_symmetrize(self._h, C.byref(h)))
        return Graph(h)

    # -- accessors ---------------------------------------------------------
    @property
    def V(self):
        return lib().gmx_graph_num_nodes(self._h)

    @property
    def E(self):
        return lib().gmx_graph_num_edges(self._h)

    def download(self, reverse=True):
        V, E = self.V, self.E
        begin = np.empty(V + 1, np.int32)
        node_idx = np.empty(E, np.int32)
        rb = rn = None
        if reverse:
            rb = np.empty(V + 1, np.int32)
            rn = np.empty(E, np.int32)
        _ck(lib().gmx_graph_download(self._h, begin.ctypes.data, node_idx.ctypes.data,
                                     rb.ctypes.data if reverse else None, rn.ctypes.data if reverse else None))
        return begin, node_idx, rb, rn

    def free(self):
        if self._h:
            lib().gmx_graph_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # -- the three kernels (mirror of the generated entry points) ----------
    def pagerank(self, e=0.001, d=0.85, max_iter=100, dtype=np.float64):
        """pagerank(G, e, d, max, G_pg_rank) -- returns (rank, stats)."""
        rank = np.empty(self.V, dtype)
        st = Stats()
        if dtype == np.float64:
            _ck(lib().gmx_pagerank_f64(self._h, e, d, max_iter, rank.ctypes.data, C.byref(st)))
        elif dtype == np.float32:
            _ck(lib().gmx_pagerank_f32(self._h, e, d, max_iter, rank.ctypes.data, C.byref(st)))
        else:
            raise GmxError("dtype must be float32 or float64")
        return rank, st.as_dict()

    def hop_dist(self, root=0):
        """hop_dist(G, G_dist, root) -- returns (dist, stats)."""
        dist = np.empty(self.V, np.int32)
        st = Stats()
        _ck(lib().gmx_hop_dist(self._h, root, dist.ctypes.data, C.byref(st)))
        return dist, st.as_dict()

    def bfs_levels(self, root=0):
        """prepare(root) + do_bfs_forward() of the BFS object -> (level[int16], unvisited = -2; number of levels)."""
        lv = np.zeros(self.V, np.int16)
        n = C.c_int32(0)
        _ck(lib().gmx_bfs_levels(self._h, int(root), lv.ctypes.data, C.byref(n)))
        return lv, n.value

    def bc(self, seeds, skip_root=False):
        """comp_BC(G, BC, Seeds) of bc.gm -> (BC[float32], stats)."""
        seeds = _i32(seeds)
        out = np.zeros(self.V, np.float32)
        st = Stats()
        _ck(lib().gmx_bc(self._h, seeds.ctypes.data if len(seeds) else None, len(seeds), int(bool(skip_root)), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def bc_batch(self, seeds, skip_root=False, width=0):
        """gmx_bc_batch: comp_BC with the seeds swept `width` at a time (0: the library's choice) -> (BC[float32], stats);
        the bytes of bc(seeds, skip_root)."""
        seeds = _i32(seeds)
        out = np.zeros(self.V, np.float32)
        st = Stats()
        _ck(lib().gmx_bc_batch(self._h, seeds.ctypes.data if len(seeds) else None, len(seeds), int(bool(skip_root)), int(width), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def bc_all(self, skip_root=True, width=0):
        """gmx_bc_all: comp_BC(G, BC) of bc_adj.gm, exact betweenness centrality with every vertex a source in node order
        -> (BC[float32], stats); the bytes of bc(arange(V), skip_root)."""
        out = np.zeros(self.V, np.float32)
        st = Stats()
        _ck(lib().gmx_bc_all(self._h, int(bool(skip_root)), int(width), out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def sssp(self, length, root=0):
        """sssp(G, dist, len, root): length[E] int32 by forward edge slot -- returns (dist[int32], stats)."""
        length = _i32(length)
        assert len(length) == self.E
        dist = np.zeros(self.V, np.int32)
        st = Stats()
        _ck(lib().gmx_sssp(self._h, int(root), length.ctypes.data if self.E else None, dist.ctypes.data, C.byref(st)))
        return dist, st.as_dict()

    def sssp_path(self, length, root=0):
        """sssp_path(G, dist, len, root, prev): length[E] int32 >= 0 by uploaded forward edge slot -- returns (dist[int32],
        prev_node[int32], prev_edge[int32], stats).  prev_* are -1 for the root and unreached vertices, otherwise the
        canonical tight in-edge (the smallest uploaded slot where every tight in-edge has positive length) and its source."""
        length = _i32(length)
        assert len(length) == self.E
        V = self.V
        dist, prev_node, prev_edge = (np.zeros(max(V, 1), np.int32) for _ in range(3))
        st = Stats()
        _ck(lib().gmx_sssp_path(self._h, int(root), length.ctypes.data if self.E else None, dist.ctypes.data,
                                prev_node.ctypes.data, prev_edge.ctypes.data, C.byref(st)))
        return dist[:V], prev_node[:V], prev_edge[:V], st.as_dict()

    def sssp_path_f64(self, cost, root=0, end=-1):
        """sssp_path(G, dist, edge_cost, root, end, prev_node, prev_edge) of sssp_path_adj.gm: cost[E] float64 >= 0 by uploaded
        forward edge slot, end = -1 for no target -- returns (dist[float64] with DBL_MAX for the unreached, prev_node[int32],
        prev_edge[int32] as uploaded slots, stats), the bytes of the reference's loop run by one thread."""
        cost = np.ascontiguousarray(cost, np.float64)
        if cost.shape != (self.E,):
            raise ValueError("cost must have one entry per edge")
        V = self.V
        dist = np.zeros(max(V, 1), np.float64)
        prev_node, prev_edge = (np.zeros(max(V, 1), np.int32) for _ in range(2))
        st = Stats()
        _ck(lib().gmx_sssp_path_f64(self._h, int(root), int(end), cost.ctypes.data if self.E else None, dist.ctypes.data,
                                    prev_node.ctypes.data, prev_edge.ctypes.data, C.byref(st)))
        return dist[:V], prev_node[:V], prev_edge[:V], st.as_dict()

    def route(self, weight):
        """gmx_route_create: weight[E] int32 >= 0 by uploaded forward edge slot -> Route, which keeps the weights on the device
        and answers (src, dst) pairs.  It borrows this graph: free it first."""
        weight = _i32(weight)
        if weight.shape != (self.E,):
            raise ValueError("weight must have one entry per edge")
        h = C.c_void_p()
        _ck(lib().gmx_route_create(self._h, weight.ctypes.data if self.E else None, C.byref(h)))
        return Route(self, h)

    def bidir_dijkstra(self, weight, src, dst):
        """bidir_dijkstra(G, Weight, src, dst, Parent, ParentEdge): returns (found, parent[int32], parent_edge[int32], stats);
        the parents are -1 off the returned route, parent_edge an uploaded forward slot."""
        weight = _i32(weight)
        if weight.shape != (self.E,):
            raise ValueError("weight must have one entry per edge")
        V = self.V
        parent, parent_edge = (np.zeros(max(V, 1), np.int32) for _ in range(2))
        found, st = C.c_int32(0), Stats()
        _ck(lib().gmx_bidir_dijkstra(self._h, weight.ctypes.data if self.E else None, int(src), int(dst), parent.ctypes.data,
                                     parent_edge.ctypes.data, C.byref(found), C.byref(st)))
        return bool(found.value), parent[:V], parent_edge[:V], st.as_dict()

    def scc(self):
        """kosaraju(G, mem): strongly connected components -- returns (comp[int32], count, stats).  comp numbers the
        components canonically: 0 .. count-1 in increasing order of each component's smallest vertex id."""
        comp = np.zeros(max(self.V, 1), np.int32)
        n, st = C.c_int64(0), Stats()
        _ck(lib().gmx_scc(self._h, comp.ctypes.data, C.byref(n), C.byref(st)))
        return comp[:self.V], int(n.value), st.as_dict()

    def wcc(self):
        """Weakly connected components -- returns (comp[int32], count, stats), numbered as scc() numbers its components.
        Any row order; a graph without the reverse CSR gives the same arrays with more work (gmx.h: GMX_WCC_*)."""
        comp = np.zeros(max(self.V, 1), np.int32)
        n, st = C.c_int64(0), Stats()
        _ck(lib().gmx_wcc(self._h, comp.ctypes.data, C.byref(n), C.byref(st)))
        return comp[:self.V], int(n.value), st.as_dict()

    KCORE_MODES = {"in": 0, "out": 1, "both": 2}

    def kcore(self, mode="in", layers=False):
        """k-core decomposition -- returns (core[int32], max_core, stats), with layers=True (core, layer[int32], max_core,
        stats).  mode "in", "out" or "both" names the slots that count as a vertex's degree; layer[v] is the round that
        removed v under the schedule in gmx.h (GMX_KCORE_*).  Any row order; "out" and "both" need the reverse CSR."""
        m = self.KCORE_MODES[mode] if isinstance(mode, str) else int(mode)
        core = np.zeros(max(self.V, 1), np.int32)
        layer = np.zeros(max(self.V, 1), np.int32) if layers else None
        k, st = C.c_int32(0), Stats()
        _ck(lib().gmx_kcore(self._h, m, core.ctypes.data, layer.ctypes.data if layers else None, C.byref(k), C.byref(st)))
        if layers:
            return core[:self.V], layer[:self.V], int(k.value), st.as_dict()
        return core[:self.V], int(k.value), st.as_dict()

    def msf(self, weight=None, components=False):
        """Minimum spanning forest of the stored slots read as undirected edges, ordered by (weight, uploaded slot) --
        returns (in_forest[bool, E] by uploaded forward edge slot, num_edges, total_weight, stats), with components=True
        (in_forest, num_edges, total_weight, comp[int32], num_comps, stats) where comp is numbered as wcc() numbers it.
        weight[E] int32 by uploaded forward edge slot, or None: all 0.  Forward CSR only, any row order (gmx.h: GMX_MSF_*)."""
        w = None
        if weight is not None:
            w = _i32(weight)
            if w.shape != (self.E,):
                raise ValueError("weight must have one entry per edge slot")
        sel = np.zeros(max(self.E, 1), np.uint8)
        comp = np.zeros(max(self.V, 1), np.int32) if components else None
        ne, tw, nc, st = C.c_int64(0), C.c_int64(0), C.c_int64(0), Stats()
        _ck(lib().gmx_msf(self._h, w.ctypes.data if w is not None and self.E else None, sel.ctypes.data if self.E else None, C.byref(ne), C.byref(tw),
                          comp.ctypes.data if components else None, C.byref(nc), C.byref(st)))
        if components:
            return sel[:self.E].astype(bool), int(ne.value), int(tw.value), comp[:self.V], int(nc.value), st.as_dict()
        return sel[:self.E].astype(bool), int(ne.value), int(tw.value), st.as_dict()

    def coloring(self, prio=None, depth=False):
        """Greedy (first-fit) vertex colouring in a fixed vertex order -- returns (color[int32], num_colors, stats), with
        depth=True (color, depth[int32], num_colors, stats).  prio[V] int32: a larger priority comes first, ties go to the
        lower id; None: largest degree (out-slots + in-slots) first.  color == 0 is the greedy maximal independent set of
        the order; depth[v] is the round that coloured v under the schedule in gmx.h (GMX_COLOR_*).  Any row order; needs
        the reverse CSR."""
        p = None
        if prio is not None:
            p = _i32(prio)
            if p.shape != (self.V,):
                raise ValueError("prio must have one entry per vertex")
        color = np.zeros(max(self.V, 1), np.int32)
        dep = np.zeros(max(self.V, 1), np.int32) if depth else None
        n, st = C.c_int32(0), Stats()
        _ck(lib().gmx_coloring(self._h, p.ctypes.data if p is not None and self.V else None, color.ctypes.data, dep.ctypes.data if depth else None,
                               C.byref(n), C.byref(st)))
        if depth:
            return color[:self.V], dep[:self.V], int(n.value), st.as_dict()
        return color[:self.V], int(n.value), st.as_dict()

    CLOSE_MODES = {"out": 0, "in": 1, "both": 2}

    def closeness(self, mode="out", sources=None):
        """Distance centralities by hop count -- returns (far[int64], reach[int32], ecc[int32], harm[uint64], stats).  mode
        "out": v's distances to the sources along out-edges (forward CSR only), "in": from the sources to v, "both": the
        slots read as undirected edges (both need the reverse CSR).  sources None: every vertex; else a list of pivots, a
        repeated one counting again.  Over the sources at distance 0 < D < infinity: reach = their number, far = sum of D,
        ecc = max of D, harm = sum of floor(2^32 / D).  All four are exact integers whose bytes no knob changes (gmx.h:
        GMX_CLOSE_*); closeness_of() and harmonic_of() derive the usual doubles."""
        m = self.CLOSE_MODES[mode] if isinstance(mode, str) else int(mode)
        src = None
        if sources is not None:
            src = _i32(sources).reshape(-1)
        n = max(self.V, 1)
        far, reach, ecc, harm = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)
        keep = np.zeros(1, np.int32)   # (a list of no sources is still a list: a non-NULL pointer)
        st = Stats()
        _ck(lib().gmx_closeness(self._h, m, None if src is None else (src if len(src) else keep).ctypes.data, 0 if src is None else len(src),
                                far.ctypes.data, reach.ctypes.data, ecc.ctypes.data, harm.ctypes.data, C.byref(st)))
        return far[:self.V], reach[:self.V], ecc[:self.V], harm[:self.V], st.as_dict()

    def communities(self, max_rounds=1000):
        """communities(G, comm): label propagation under the canonical tie rule and schedule (gmx.h) -- returns
        (comm[int32], rounds, converged, stats).  comm holds vertex ids; converged is 1 when comm is a fixpoint."""
        comm = np.zeros(max(self.V, 1), np.int32)
        rounds, conv, st = C.c_int32(0), C.c_int32(0), Stats()
        _ck(lib().gmx_communities(self._h, int(max_rounds), comm.ctypes.data, C.byref(rounds), C.byref(conv), C.byref(st)))
        return comm[:self.V], int(rounds.value), int(conv.value), st.as_dict()

    def _pf_range(self, v_lo, v_hi):
        v_lo, v_hi = int(v_lo), int(self.V if v_hi is None else v_hi)
        if not 0 <= v_lo <= v_hi <= self.V:
            raise GmxError("vertex range [%d, %d) outside [0, %d]" % (v_lo, v_hi, self.V))
        return v_lo, v_hi

    def potential_friends(self, v_lo=0, v_hi=None):
        """potential_friends(G, potFriend) for the vertices v_lo <= v < v_hi (v_hi None: V) -- returns (pf_begin[int64],
        pf_idx[int32], stats): a CSR whose row i is PF(v_lo + i), the out-neighbours of v's out-neighbours that are neither v
        nor out-neighbours of v, ascending and distinct.  One sizing call, then the filling call; stats are the latter's."""
        v_lo, v_hi = self._pf_range(v_lo, v_hi)
        begin = np.zeros(v_hi - v_lo + 1, np.int64)
        total, st = C.c_int64(0), Stats()
        _ck(lib().gmx_potential_friends(self._h, v_lo, v_hi, begin.ctypes.data, None, 0, C.byref(total), C.byref(st)))
        idx = np.zeros(max(total.value, 1), np.int32)
        _ck(lib().gmx_potential_friends(self._h, v_lo, v_hi, begin.ctypes.data, idx.ctypes.data, total.value, C.byref(total), C.byref(st)))
        return begin, idx[:total.value], st.as_dict()

    def potential_friend_counts(self, v_lo=0, v_hi=None):
        """|PF(v)| for v_lo <= v < v_hi as int64[v_hi - v_lo]: the sizing call only.  The run statistics are left in last_stats."""
        v_lo, v_hi = self._pf_range(v_lo, v_hi)
        begin = np.zeros(v_hi - v_lo + 1, np.int64)
        st = Stats()
        _ck(lib().gmx_potential_friends(self._h, v_lo, v_hi, begin.ctypes.data, None, 0, None, C.byref(st)))
        self.last_stats = st.as_dict()
        return np.diff(begin)

    def avg_teen_cnt(self, age, K):
        """avg_teen_cnt(G, age, teen_cnt, K) -- returns (avg float32, teen_cnt[int32], stats)."""
        age = _i32(age)
        assert len(age) == self.V
        cnt = np.zeros(self.V, np.int32)
        avg, st = C.c_float(0), Stats()
        _ck(lib().gmx_avg_teen_cnt(self._h, age.ctypes.data if self.V else None, int(K), cnt.ctypes.data if self.V else None,
                                   C.byref(avg), C.byref(st)))
        return np.float32(avg.value), cnt, st.as_dict()

    def conduct(self, member, num):
        """conduct(G, member, num) -- returns (float32, stats)."""
        member = _i32(member)
        assert len(member) == self.V
        res, st = C.c_float(0), Stats()
        _ck(lib().gmx_conduct(self._h, member.ctypes.data if self.V else None, int(num), C.byref(res), C.byref(st)))
        return np.float32(res.value), st.as_dict()

    def edge_order(self):
        """e_idx2idx after an upload with GMX_GRAPH_SORT_ROWS: uploaded slot of every slot of the sorted rows;
        None when the upload was already in order (identity)."""
        out = np.zeros(self.E, np.int32)
        ident = C.c_int(1)
        _ck(lib().gmx_graph_edge_order(self._h, out.ctypes.data if self.E else None, C.byref(ident)))
        return None if ident.value else out

    def reverse_edge_map(self):
        """e_rev2idx: forward slot mirrored by each reverse-CSR slot."""
        out = np.zeros(self.E, np.int32)
        _ck(lib().gmx_graph_reverse_edge_map(self._h, out.ctypes.data))
        return out

    def common_nbrs(self, s, d):
        """The items gm_common_neighbor_iter(G, s, d) yields, in order."""
        n = C.c_int64(0)
        _ck(lib().gmx_common_nbrs(self._h, int(s), int(d), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        _ck(lib().gmx_common_nbrs(self._h, int(s), int(d), out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def common_nbr_counts(self, src, dst):
        src, dst = _i32(src), _i32(dst)
        out = np.zeros(max(len(src), 1), np.int64)
        _ck(lib().gmx_common_nbr_counts(self._h, src.ctypes.data, dst.ctypes.data, len(src), out.ctypes.data))
        return out[:len(src)]

    def triangle_counting_cn(self):
        """Triangle counting written with the common-neighbour iterator -- returns (T, stats)."""
        t, st = C.c_int64(0), Stats()
        _ck(lib().gmx_triangle_counting_cn(self._h, C.byref(t), C.byref(st)))
        return t.value, st.as_dict()

    def adamic_adar(self):
        """adamicAdar(G, aa): aa[float64, E] by uploaded forward edge slot -- the sum of 1 / log(outdeg n) over the common
        neighbours n of the edge's two ends, as the iterator yields them.  The run statistics are left in last_stats."""
        aa = np.zeros(max(self.E, 1), np.float64)
        st = Stats()
        _ck(lib().gmx_adamic_adar(self._h, aa.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        return aa[:self.E]

    def v_cover(self):
        """v_cover(G, select): the greedy vertex cover as one thread of the reference runs it (ties to the lowest slot) --
        returns (select[bool, E] by uploaded forward edge slot, covered, stats).  Needs the reverse CSR; any row order."""
        sel = np.zeros(max(self.E, 1), np.uint8)
        cov, st = C.c_int32(0), Stats()
        _ck(lib().gmx_v_cover(self._h, sel.ctypes.data if self.E else None, C.byref(cov), C.byref(st)))
        return sel[:self.E].astype(bool), int(cov.value), st.as_dict()

    def random_bipartite_matching(self, is_left):
        """random_bipartite_matching(G, isLeft, Match): the maximal matching as one thread of the reference runs it (a right
        takes its largest proposing left, a left its largest replying right) -- returns (match[int32, V] with -1 for the
        unmatched, count, stats).  Only rows of left vertices are read, forward CSR only, any row order."""
        left = np.ascontiguousarray(np.asarray(is_left) != 0, np.uint8)
        if left.shape != (self.V,):
            raise ValueError("is_left must have one entry per vertex")
        match = np.full(max(self.V, 1), -1, np.int32)
        cnt, st = C.c_int32(0), Stats()
        _ck(lib().gmx_random_bipartite_matching(self._h, left.ctypes.data if self.V else None, match.ctypes.data if self.V else None,
                                                C.byref(cnt), C.byref(st)))
        return match[:self.V], int(cnt.value), st.as_dict()

    def random_walk_sampling(self, p_size, p_jump, num_tokens, rng_state, max_rounds=INT_MAX):
        """parallel_random_walk_jump_sampling(G, p_size, p_jump, num_tokens, Selected) as one thread of the reference runs it on
        the 48-bit stream that starts at rng_state -- returns (selected[uint8, V], token[int32, V], count, rounds, state after,
        stats).  Forward CSR only, any row order."""
        sel = np.zeros(max(self.V, 1), np.uint8)
        tok = np.zeros(max(self.V, 1), np.int32)
        x, cnt, rounds, st = C.c_uint64(rng_state), C.c_int64(0), C.c_int32(0), Stats()
        _ck(lib().gmx_random_walk_sampling(self._h, p_size, p_jump, num_tokens, max_rounds, C.byref(x), sel.ctypes.data, tok.ctypes.data,
                                           C.byref(cnt), C.byref(rounds), C.byref(st)))
        return sel[:self.V], tok[:self.V], int(cnt.value), int(rounds.value), int(x.value), st.as_dict()

    def node_sampling(self, by_degree, N, rng_state):
        """random_node_sampling (by_degree = 0) / random_degree_node_sampling (by_degree = 1): vertex v takes draw v + 1 of
        the stream -- returns (selected[uint8, V], count, state after, stats)."""
        sel = np.zeros(max(self.V, 1), np.uint8)
        x, cnt, st = C.c_uint64(rng_state), C.c_int64(0), Stats()
        _ck(lib().gmx_node_sampling(self._h, 1 if by_degree else 0, N, C.byref(x), sel.ctypes.data if self.V else None, C.byref(cnt), C.byref(st)))
        return sel[:self.V], int(cnt.value), int(x.value), st.as_dict()

    def triangle_counting(self, part=0, nparts=1):
        """triangle_counting(G) -- returns (T, stats); with nparts > 1 the share of one part of the edge slots."""
        t = C.c_int64(0)
        st = Stats()
        _ck(lib().gmx_triangle_counting_part(self._h, part, nparts, C.byref(t), C.byref(st)))
        return t.value, st.as_dict()

    def triangle_counting_directed(self, part=0, nparts=1):
        """triangle_counting_directed(G): the slot pairs (u, w), u < w, of every row whose two ends are joined by an edge in
        either direction -- returns (T, stats); with nparts > 1 the share of one part of the work items.  Any row order."""
        t = C.c_int64(0)
        st = Stats()
        _ck(lib().gmx_triangle_counting_directed_part(self._h, part, nparts, C.byref(t), C.byref(st)))
        return t.value, st.as_dict()

    def clustering(self, tri=True, deg=True, lcc=True):
        """Per-vertex triangle counts and local clustering coefficients of the stored slots read as an undirected simple graph
        -- returns (tri[int64], deg[int32], lcc[float64], triangles, wedges, stats); an array not asked for is None.  tri[v] is
        the number of triangles through v, deg[v] its distinct neighbours, lcc[v] = 2 tri / (deg (deg - 1)) (0.0 below deg 2),
        triangles = sum(tri) / 3 and wedges = sum(deg (deg - 1) / 2): transitivity is 3 * triangles / wedges, the average
        clustering coefficient lcc.mean().  Forward CSR only, any row order (gmx.h: GMX_LCC_*)."""
        n = max(self.V, 1)
        t = np.zeros(n, np.int64) if tri else None
        d = np.zeros(n, np.int32) if deg else None
        c = np.zeros(n, np.float64) if lcc else None
        T, W, st = C.c_int64(0), C.c_int64(0), Stats()
        _ck(lib().gmx_clustering(self._h, t.ctypes.data if tri else None, d.ctypes.data if deg else None, c.ctypes.data if lcc else None,
                                 C.byref(T), C.byref(W), C.byref(st)))
        V = self.V
        return (t[:V] if tri else None, d[:V] if deg else None, c[:V] if lcc else None, int(T.value), int(W.value), st.as_dict())

    def biconnected(self, bridges=True, artic=True, blocks=True, tecc=True):
        """Bridges, articulation points, biconnected components and 2-edge-connected components of the stored slots read as an
        undirected simple graph -- returns (bridge[bool, E] and block[int32, E] by uploaded forward slot, artic[bool, V],
        tecc[int32, V], in the order bridge, artic, block, tecc, then num_blocks, num_bridges, num_artic, num_tecc, stats); an
        array not asked for is None and is not built.  block is -1 at self-loop slots, its ids increase with each block's
        smallest uploaded slot; tecc is numbered as wcc() numbers components.  Any row order; needs the reverse CSR (gmx.h:
        GMX_BICC_*)."""
        V, E = self.V, self.E
        br = np.zeros(max(E, 1), np.uint8) if bridges else None
        ar = np.zeros(max(V, 1), np.uint8) if artic else None
        bl = np.full(max(E, 1), -1, np.int32) if blocks else None
        te = np.zeros(max(V, 1), np.int32) if tecc else None
        n = [C.c_int64(0) for _ in range(4)]
        st = Stats()
        _ck(lib().gmx_biconnected(self._h, br.ctypes.data if bridges else None, ar.ctypes.data if artic else None, bl.ctypes.data if blocks else None,
                                  te.ctypes.data if tecc else None, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), C.byref(n[3]), C.byref(st)))
        return (br[:E].astype(bool) if bridges else None, ar[:V].astype(bool) if artic else None, bl[:E] if blocks else None,
                te[:V] if tecc else None, int(n[0].value), int(n[1].value), int(n[2].value), int(n[3].value), st.as_dict())

    def ktruss(self, truss=True, support=True):
        """k-truss decomposition and per-edge triangle support of the stored slots read as an undirected simple graph -- returns
        (truss[int32, E], support[int32, E], max_truss, num_edges, stats), both arrays by uploaded forward slot; an array not
        asked for is None and is not built.  support[e] is the number of triangles through the slot's edge, truss[e] the largest
        k such that the edge lies in a subgraph whose every edge is in at least k - 2 triangles of that subgraph (at least 2);
        every slot of one undirected edge carries the same values and a self-loop slot carries 0.  max_truss is the largest
        truss number, num_edges the number of undirected edges, stats["vertices_reached"] the edges of the largest truss number
        and stats["iterations"] the peeling rounds.  truss=False is the cheap triangles-per-edge query: nothing is peeled and
        max_truss is 0.  Forward CSR only, any row order (gmx.h: GMX_KTRUSS_*)."""
        E = self.E
        t = np.zeros(max(E, 1), np.int32) if truss else None
        s = np.zeros(max(E, 1), np.int32) if support else None
        k, n, st = C.c_int32(0), C.c_int64(0), Stats()
        _ck(lib().gmx_ktruss(self._h, t.ctypes.data if truss else None, s.ctypes.data if support else None, C.byref(k), C.byref(n), C.byref(st)))
        return (t[:E] if truss else None, s[:E] if support else None, int(k.value), int(n.value), st.as_dict())

    def kclique(self, k, per_vertex=True):
        """k-clique counts of the stored slots read as an undirected simple graph, 3 <= k <= 8 -- returns (count[int64, V] or
        None, cliques, stats).  cliques is the number of k-element vertex sets that are pairwise adjacent, count[v] the number
        of those that contain v: count.sum() == k * cliques, and k = 3 gives clustering()'s tri and triangles.
        per_vertex=False is the cheap total-only query: count is None and is not built.  Sums are 64-bit and wrap modulo 2^64.
        Forward CSR only, any row order (gmx.h: GMX_KCLIQUE_*)."""
        V = self.V
        c = np.zeros(max(V, 1), np.int64) if per_vertex else None
        n, st = C.c_int64(0), Stats()
        _ck(lib().gmx_kclique(self._h, int(k), c.ctypes.data if per_vertex else None, C.byref(n), C.byref(st)))
        return (c[:V] if per_vertex else None, int(n.value), st.as_dict())

    def squares(self, per_vertex=True):
        """4-cycle (square) counts of the stored slots read as an undirected simple graph -- returns (count[int64, V] or None,
        squares, stats).  squares is the number of cycles a - b - c - d - a on four distinct vertices (chords allowed: K4 holds
        three; on a bipartite graph its butterflies), count[v] the number of those through v: count.sum() == 4 * squares.
        per_vertex=False is the cheap total-only query: count is None and is not built.  Exact while 2 * count[v] < 2^63.
        stats["edges_examined"] is the number of wedges walked.  Forward CSR only, any row order (gmx.h: GMX_SQUARES_*)."""
        V = self.V
        c = np.zeros(max(V, 1), np.int64) if per_vertex else None
        n, st = C.c_int64(0), Stats()
        _ck(lib().gmx_squares(self._h, c.ctypes.data if per_vertex else None, C.byref(n), C.byref(st)))
        return (c[:V] if per_vertex else None, int(n.value), st.as_dict())

    def graphlets(self, per_vertex=True, induced=True):
        """The census of the connected subgraphs on 2, 3 and 4 vertices of the stored slots read as an undirected simple graph --
        returns (gdv[int64, V x 15] or None, totals[int64, 9], stats).  gdv[v, k] is the number of subgraphs in which v sits at
        orbit k (numbered as in ORCA: 0 degree, 1 - 2 path on 3, 3 triangle, 4 - 5 path on 4, 6 - 7 claw, 8 4-cycle, 9 - 11 paw,
        12 - 13 diamond, 14 K4), totals[j] the number of graphlets G0 .. G8.  induced=True counts induced subgraphs,
        induced=False subgraphs (the convention of squares(): gdv[:, 8] and gdv[:, 14] are squares()'s and kclique(4)'s
        counts).  per_vertex=False is the cheap totals-only query: gdv is None and no per-vertex kernel runs.
        stats["edges_examined"] is the number of triangles walked.  Forward CSR only, any row order (gmx.h: GMX_GRAPHLETS_*)."""
        V = self.V
        gdv = np.zeros((max(V, 1), 15), np.int64) if per_vertex else None
        totals, st = np.zeros(9, np.int64), Stats()
        _ck(lib().gmx_graphlets(self._h, 1 if induced else 0, gdv.ctypes.data if per_vertex else None, totals.ctypes.data, C.byref(st)))
        return (gdv[:V] if per_vertex else None, totals, st.as_dict())

    def louvain(self, weight=None, max_levels=32, max_rounds=64):
        """Louvain modularity communities of the stored slots read as undirected edges -- returns (comm[int32], num_comms,
        num_levels, modularity, intra, stats).  weight[E] int32 >= 1 by uploaded forward edge slot, or None: all 1; a repeated
        slot is another edge and a self loop counts twice on the diagonal.  comm is numbered as wcc() numbers components,
        num_levels counts the levels that kept a move, modularity = Qnum / m2^2 from the exact 128-bit numerator and intra is
        the weight inside the communities (both directions).  All decisions are integer: the result is byte-identical to the
        one-thread schedule in gmx.h.  Forward CSR only, any row order (gmx.h: GMX_LOUVAIN_*)."""
        w = None
        if weight is not None:
            w = _i32(weight)
            if w.shape != (self.E,):
                raise ValueError("weight must have one entry per edge slot")
        V = self.V
        c = np.zeros(max(V, 1), np.int32)
        nc, nl, q, intra, st = C.c_int32(0), C.c_int32(0), C.c_double(0.0), C.c_int64(0), Stats()
        _ck(lib().gmx_louvain(self._h, w.ctypes.data if w is not None and self.E else None, int(max_levels), int(max_rounds), c.ctypes.data,
                              C.byref(nc), C.byref(nl), C.byref(q), C.byref(intra), C.byref(st)))
        return c[:V], int(nc.value), int(nl.value), float(q.value), int(intra.value), st.as_dict()


def closeness_of(far, reach, wasserman_faust=False):
    """Closeness from Graph.closeness()'s integers: reach / far (0 where nothing is reached); with wasserman_faust=True
    scaled by reach / (V - 1), the form that compares vertices of different components."""
    far, reach = np.asarray(far, np.float64), np.asarray(reach, np.float64)
    c = np.divide(reach, far, out=np.zeros_like(far), where=far > 0)
    if wasserman_faust and len(c) > 1:
        c = c * reach / (len(c) - 1)
    return c


def harmonic_of(harm):
    """Harmonic centrality from Graph.closeness()'s fixed point: harm / 2^32 (from below by less than reach * 2^-32)."""
    return np.asarray(harm, np.uint64).astype(np.float64) / 4294967296.0


def path_from_prev(prev_node, begin, end):
    """get_path of sssp_path.gm on Graph.sssp_path's prev_node: the vertices begin .. end of the tree path, or [] when end
    has no predecessor (unreached, or the root itself).  begin must lie on end's path to the root."""
    path = []
    if prev_node[end] < 0:
        return path
    t = int(end)
    while t != begin:
        path.append(t)
        t = int(prev_node[t])
        if t < 0 or len(path) > len(prev_node):
            raise GmxError("begin %d is not on the path from the root to %d" % (begin, end))
    path.append(t)
    return path[::-1]


def default_pr_options(V, nranks=1):
    return int(lib().gmx_pr_default_options(V, nranks))


class DevArray:
    """A raw device pointer exposed through __cuda_array_interface__ so that torch can wrap it
    (torch.as_tensor(DevArray(...), device='cuda')) for torch.distributed collectives."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class BfsState:
    """Device-resident hop_dist stepping state (gmx_bfs_*) for one rank of nranks (replicated graph)."""

    def __init__(self, graph, rank=0, nranks=1):
        self.graph = graph
        self.rank, self.nranks = rank, nranks
        h = C.c_void_p()
        _ck(lib().gmx_bfs_create(graph._h, rank, nranks, C.byref(h)))
        self._h = h

    def start(self, root):
        _ck(lib().gmx_bfs_start(self._h, int(root)))

    def step_begin(self):
        """Runs the local part of the next level; True if the found-bitmap slices have to be exchanged."""
        need = C.c_int(0)
        _ck(lib().gmx_bfs_step_begin(self._h, C.byref(need)))
        return bool(need.value)

    def found_bitmap(self):
        """(whole bitmap as DevArray of int64 words, slice offset, slice length) -- words of 64 vertices."""
        p, tot, off, n = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _ck(lib().gmx_bfs_found_bitmap(self._h, C.byref(p), C.byref(tot), C.byref(off), C.byref(n)))
        return DevArray(p.value, tot.value, "<i8"), off.value, n.value

    def step_end(self):
        n = C.c_int64(0)
        _ck(lib().gmx_bfs_step_end(self._h, C.byref(n)))
        return n.value

    def download(self):
        out = np.zeros(self.graph.V, np.int32)
        st = Stats()
        _ck(lib().gmx_bfs_download(self._h, out.ctypes.data, C.byref(st)))
        return out, st.as_dict()

    def free(self):
        if self._h:
            lib().gmx_bfs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Handles(list):
    """ipc_handles() of a rank: the replica handles as list items, the packed-exchange extras as attributes (picklable)."""

    def __init__(self, *a):
        super().__init__(*a)
        self.landing = []
        self.packed = None

    def __reduce__(self):
        return (_rebuild_handles, (list(self), self.landing, self.packed))


def _rebuild_handles(items, landing, packed):
    h = _Handles(items)
    h.landing, h.packed = landing, packed
    return h


class PageRankState:
    """Device-resident PageRank stepping state (gmx_pr_*) for one rank of nranks."""

    def __init__(self, graph, elem_bytes=4, rank=0, nranks=1, options=GMX_PR_RELABEL):
        self.graph = graph
        self.elem = elem_bytes
        self.rank, self.nranks = rank, nranks
        h = C.c_void_p()
        _ck(lib().gmx_pr_create(graph._h, elem_bytes, rank, nranks, options, C.byref(h)))
        self._h = h

    def reset(self, d=0.85):
        _ck(lib().gmx_pr_reset(self._h, d))

    def step(self, stream=None):
        _ck(lib().gmx_pr_step(self._h, stream))

    # ---- peer push (gmx.h: exchange by direct copies into the peers' replicas, packed when the plan has the lists) ----
    def packed_info(self):
        """{"send": [...], "recv": [...], "offset": [...]} (elements per peer) of the packed exchange, or None when the
        plan has no lists (one rank, or not the degree order)."""
        n = self.nranks
        a, b, c = (C.c_int64 * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
        if lib().gmx_pr_packed_info(self._h, a, b, c) != 0:
            return None
        return {"send": list(a), "recv": list(b), "offset": list(c)}

    def _buffers(self, landing):
        b0, b1, n = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _ck((lib().gmx_pr_recv_buffers if landing else lib().gmx_pr_contrib_buffers)(self._h, C.byref(b0), C.byref(b1), C.byref(n)))
        return b0, b1

    def ipc_handles(self):
        """What the other ranks need to push into this one: hipIpc handles (bytes) of the two contribution replicas
        [0], [1]; with a packed plan also ["landing"] (handles of the two landing zones) and ["packed"] (packed_info())."""
        out = _Handles()
        for b in self._buffers(False):
            h = C.create_string_buffer(IPC_HANDLE_BYTES)
            _ck(lib().gmx_ipc_export(b, h))
            out.append(h.raw)
        info = self.packed_info()
        if info is not None and os.environ.get("GMX_PUSH_PACKED", "1") != "0":
            out.packed = info
            for b in self._buffers(True):
                h = C.create_string_buffer(IPC_HANDLE_BYTES)
                _ck(lib().gmx_ipc_export(b, h))
                out.landing.append(h.raw)
        return out

    def _register_peers(self, ptrs, land, infos):
        _ck(lib().gmx_pr_set_peers(self._h, ptrs[0], ptrs[1]))
        self.packed_push = False
        if land is not None:
            off, cnt = (C.c_int64 * self.nranks)(), (C.c_int64 * self.nranks)()
            for r in range(self.nranks):
                if r != self.rank:
                    off[r], cnt[r] = infos[r]["offset"][self.rank], infos[r]["recv"][self.rank]
            _ck(lib().gmx_pr_set_peers_packed(self._h, land[0], land[1], off, cnt))
            self.packed_push = True

    def set_peers(self, handles):
        """handles[r] = rank r's ipc_handles() (own entry ignored): map them and register the pointers.  The packed
        push is used when every rank offers landing zones."""
        ptrs = [(C.c_void_p * self.nranks)(), (C.c_void_p * self.nranks)()]
        packed = self.packed_info() is not None and all(getattr(h, "packed", None) is not None for h in handles)
        land = [(C.c_void_p * self.nranks)(), (C.c_void_p * self.nranks)()] if packed else None
        self._peer_maps = []
        for r, hs in enumerate(handles):
            if r == self.rank:
                continue
            for b in (0, 1):
                for dst, src in ((ptrs, hs), (land, hs.landing if packed else None)):
                    if dst is None:
                        continue
                    q = C.c_void_p()
                    _ck(lib().gmx_ipc_open(C.create_string_buffer(src[b], IPC_HANDLE_BYTES), C.byref(q)))
                    dst[b][r] = q.value
                    self._peer_maps.append(q.value)
        self._register_peers(ptrs, land, [getattr(h, "packed", None) for h in handles])

    def set_peers_local(self, states):
        """The same wiring for rank states that live in THIS process (tests, one-GPU rehearsals): raw device pointers."""
        ptrs = [(C.c_void_p * self.nranks)(), (C.c_void_p * self.nranks)()]
        infos = [s.packed_info() for s in states]
        packed = all(i is not None for i in infos) and os.environ.get("GMX_PUSH_PACKED", "1") != "0"
        land = [(C.c_void_p * self.nranks)(), (C.c_void_p * self.nranks)()] if packed else None
        for r, st in enumerate(states):
            if r == self.rank:
                continue
            for dst, bufs in ((ptrs, st._buffers(False)), (land, st._buffers(True) if packed else None)):
                if dst is not None:
                    dst[0][r], dst[1][r] = bufs[0].value, bufs[1].value
        self._register_peers(ptrs, land, infos)

    def push_chunk(self, chunk, stream=None):
        if getattr(self, "packed_push", False):
            _ck(lib().gmx_pr_push_packed(self._h, int(chunk), stream))
        else:
            _ck(lib().gmx_pr_push_chunk(self._h, chunk, stream))

    def push_current(self, stream=None):
        if getattr(self, "packed_push", False):
            _ck(lib().gmx_pr_push_packed(self._h, -1, stream))
        else:
            _ck(lib().gmx_pr_push_current(self._h, stream))

    def unpack(self, chunk=-1, stream=None):
        """After the barrier that follows the pushes: scatter what the peers packed (chunk, or -1 = everything) into the
        replica the next step reads.  Nothing to do for the plain push."""
        if getattr(self, "packed_push", False):
            _ck(lib().gmx_pr_unpack(self._h, int(chunk), stream))

    def recv_list(self, r):
        """DevArray of the positions (inside rank r's range) this rank reads (packed plans)."""
        p, n = C.c_void_p(), C.c_int64(0)
        _ck(lib().gmx_pr_recv_list(self._h, int(r), C.byref(p), C.byref(n)))
        return DevArray(p.value, n.value, "<i4")

    def exchange_bytes(self):
        """Bytes this rank sends per step: the packed lists if they are in use, else the exchanged prefix to every peer."""
        if getattr(self, "packed_push", False):
            return sum(self.packed_info()["send"]) * self.elem
        return self.exchange_count() * (self.nranks - 1) * self.elem

    def push_join(self, stream=None):
        _ck(lib().gmx_pr_push_join(self._h, stream))

    def push_join_chunk(self, chunk, stream=None):
        """`stream` waits for the copies of one chunk only."""
        _ck(lib().gmx_pr_push_join_chunk(self._h, int(chunk), stream))

    def gather_classes(self):
        """2 when the step can be pipelined (every in-edge binned: step_gather(0/1) ahead of step_chunk), else 0."""
        n = C.c_int(0)
        _ck(lib().gmx_pr_gather_classes(self._h, C.byref(n)))
        return n.value

    def gather_items(self, tile_class):
        n = C.c_int64(0)
        _ck(lib().gmx_pr_gather_items(self._h, int(tile_class), C.byref(n)))
        return n.value

    def step_gather(self, tile_class, stream=None):
        _ck(lib().gmx_pr_step_gather(self._h, int(tile_class), stream))

    def set_chunks(self, chunks):
        _ck(lib().gmx_pr_set_chunks(self._h, int(chunks)))
        return self.num_chunks()

    def num_chunks(self):
        n = C.c_int(0)
        _ck(lib().gmx_pr_num_chunks(self._h, C.byref(n)))
        return n.value

    def chunk_range(self, chunk):
        off, cnt = C.c_int64(0), C.c_int64(0)
        _ck(lib().gmx_pr_chunk_range(self._h, chunk, C.byref(off), C.byref(cnt)))
        return off.value, cnt.value

    def step_chunk(self, chunk, stream=None):
        _ck(lib().gmx_pr_step_chunk(self._h, chunk, stream))

    def contrib_next_full(self):
        p, n = C.c_void_p(), C.c_int64(0)
        _ck(lib().gmx_pr_contrib_next_full(self._h, C.byref(p), C.byref(n)))
        return DevArray(p.value, n.value, self._typestr())

    def diff(self, stream=None):
        v = C.c_double(0)
        _ck(lib().gmx_pr_diff(self._h, stream, C.byref(v)))
        return v.value

    def _typestr(self):
        return "<f4" if self.elem == 4 else "<f8"

    def contrib_slice(self):
        p, n = C.c_void_p(), C.c_int64(0)
        _ck(lib().gmx_pr_contrib_slice(self._h, C.byref(p), C.byref(n)))
        return DevArray(p.value, n.value, self._typestr())

    def contrib_full(self):
        p, n = C.c_void_p(), C.c_int64(0)
        _ck(lib().gmx_pr_contrib_full(self._h, C.byref(p), C.byref(n)))
        return DevArray(p.value, n.value, self._typestr())

    def exchange_count(self):
        n = C.c_int64(0)
        _ck(lib().gmx_pr_exchange_count(self._h, C.byref(n)))
        return n.value

    def diff_dev(self):
        p = C.c_void_p()
        _ck(lib().gmx_pr_diff_ptr(self._h, C.byref(p)))
        return DevArray(p.value, 1, "<f8")

    def download(self, out=None):
        V = self.graph.V
        dt = np.float32 if self.elem == 4 else np.float64
        if out is None:
            out = np.zeros(V, dt)
        _ck(lib().gmx_pr_download(self._h, out.ctypes.data))
        return out

    def timing(self, enable=True):
        _ck(lib().gmx_pr_timing(self._h, int(enable)))

    def kernel_time(self):
        """(launches, mean_ms) of the dominant kernel since timing(True), hipEvents on its stream."""
        n, ms = C.c_int32(0), C.c_double(0)
        _ck(lib().gmx_pr_kernel_time(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def kernel_name(self):
        return lib().gmx_pr_kernel_name(self._h).decode()

    def cold_info(self):
        """(hot ids per rank range, binned edges, items of phase 2) of the binned part; hot_ids = -1 without one."""
        t, e, p = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _ck(lib().gmx_pr_cold_info(self._h, C.byref(t), C.byref(e), C.byref(p)))
        return {"hot_ids": t.value, "cold_edges": e.value, "padded_items": p.value}

    def cold_shape(self):
        """Which paths a step of the binned part takes (gmx_pr_cold_shape: host arithmetic on the plan's work lists).
        groups / supersteps are keyed by form (PR_COLD_FORMS), tiles_by_mode by PR_COLD_TILE_MODES; supersteps[form] is
        the set of whole super-step counts its phase-1 segments run (31 stands for 31 or more)."""
        s = PrColdShape()
        _ck(lib().gmx_pr_cold_shape(self._h, C.byref(s)))
        return {"groups": dict(zip(PR_COLD_FORMS, s.groups)),
                "supersteps": {f: {n for n in range(32) if m >> n & 1} for f, m in zip(PR_COLD_FORMS, s.supersteps)},
                "items2_sole": s.items2_sole, "items2_chunk": s.items2_chunk, "bins_few": s.bins_few, "bins_many": s.bins_many,
                "tiles_by_mode": dict(zip(PR_COLD_TILE_MODES, s.tiles_by_mode)), "fused": bool(s.fused)}

    def work(self):
        e, r, b = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _ck(lib().gmx_pr_work(self._h, C.byref(e), C.byref(r), C.byref(b)))
        return {"edges": e.value, "rows": r.value, "algorithmic_bytes": b.value}

    def free(self):
        if self._h:
            lib().gmx_pr_free(self._h)     # drains the copy streams first
            self._h = None
            for q in getattr(self, "_peer_maps", []):
                lib().gmx_ipc_close(q)
            self._peer_maps = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
