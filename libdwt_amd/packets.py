"""Wavelet packet transforms of row and image batches (include/libdwt_hip.h): every node is split again at
every level, not only the L node.  A submodule of its own: import it as ``from libdwt_amd import packets``.

    packets.wp1d_batch(dwt.CDF97_S, False, x, x, 4 * N, 4, n_lines, N, levels)   # in place, leaves in natural order
    packets.wp_features1d_batch("wps", x, 4 * N, 4, n_lines, N, levels, packets.FREQUENCY, fv, 1 << levels)
    tree = packets.wp_joint_basis(dwt.CDF97_S, packets.COST_SHANNON, 0.0, x, 4 * N, 4, n_lines, N, levels)   # one tree for all rows
    packets.wp_tree1d_batch(dwt.CDF97_S, False, x, x, 4 * N, 4, n_lines, N, levels, tree, 0)             # 
    qtree = packets.wp_joint_qtree(dwt.CDF97_S, packets.COST_SHANNON, 0.0, img, 4 * W * H, batch, 4 * W, 4, W, H, levels)
    packets.wp_tree2d_batch(dwt.CDF97_S, False, img, img, 4 * W * H, batch, 4 * W, 4, W, H, levels, qtree)   # 

Pointers are numpy arrays, torch tensors or integer addresses, host or device memory, as everywhere in libdwt_amd.
"""
import ctypes as C

from . import CDF53_S, CDF97_S, INTERP53_S, DwtError, _addr, _check, feature_mask, lib

_I, _P, _S, _F = C.c_int, C.c_void_p, C.c_size_t, C.c_float
_IP = C.POINTER(_I)

WAVELETS = (CDF97_S, CDF53_S, INTERP53_S)
NATURAL, FREQUENCY = 0, 1  # node order of the feature entries
MAX_LEVELS_2D = 8
MAX_FEATURE_NODES = 96  # FEAT_MAX_BANDS: level <= 6 in 1-D, <= 3 in 2-D
TREE_MAX_LEVELS, TREE_WORDS = 10, 32  # DWT_HIP_WP_TREE_MAX_LEVELS, DWT_HIP_WP_TREE_WORDS
COST_SHANNON, COST_LOG_ENERGY, COST_LP, COST_THRESHOLD = 0, 1, 2, 3  # enum dwt_hip_wp_cost

lib.dwt_hip_wp_nodes.argtypes = [_I, _I, _IP, _IP]
lib.dwt_hip_wp_nodes.restype = _I
lib.dwt_hip_wp_freq_order.argtypes = [_I, _IP]
lib.dwt_hip_wp_freq_order.restype = _I
lib.dwt_hip_wp1d_batch.argtypes = [_I, _I, _P, _P, _S, _S, _I, _I, _I]
lib.dwt_hip_wp1d_batch.restype = _I
lib.dwt_hip_wp2d_batch.argtypes = [_I, _I, _P, _P, _S, _I, _I, _I, _I, _I, _I]
lib.dwt_hip_wp2d_batch.restype = _I
lib.dwt_hip_wp_features1d_batch.argtypes = [C.c_uint, _P, _S, _S, _I, _I, _I, _I, _F, _P, _S]
lib.dwt_hip_wp_features1d_batch.restype = _I
lib.dwt_hip_wp_features2d_batch.argtypes = [C.c_uint, _P, _S, _I, _I, _I, _I, _I, _I, _F, _P, _S]
lib.dwt_hip_wp_features2d_batch.restype = _I
lib.dwt_hip_wp_best_tree.argtypes = [_I, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
lib.dwt_hip_wp_best_tree.restype = _I
lib.dwt_hip_wp_tree_leaves.argtypes = [_I, _I, C.POINTER(C.c_uint32), _IP, _IP, _IP, _IP]
lib.dwt_hip_wp_tree_leaves.restype = _I
lib.dwt_hip_wp_best1d_batch.argtypes = [_I, _I, _F, _P, _P, _S, _S, _I, _I, _I, _P, _S, _P, _P, _S]
lib.dwt_hip_wp_best1d_batch.restype = _I
lib.dwt_hip_wp_tree1d_batch.argtypes = [_I, _I, _P, _P, _S, _S, _I, _I, _I, _P, _S]
lib.dwt_hip_wp_tree1d_batch.restype = _I
QTREE_MAX_LEVELS, QTREE_WORDS = 5, 16  # DWT_HIP_WP_QTREE_MAX_LEVELS, DWT_HIP_WP_QTREE_WORDS
lib.dwt_hip_wp_best_qtree.argtypes = [_I, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
lib.dwt_hip_wp_best_qtree.restype = _I
lib.dwt_hip_wp_qtree_leaves.argtypes = [_I, _I, _I, C.POINTER(C.c_uint32)] + [_IP] * 7
lib.dwt_hip_wp_qtree_leaves.restype = _I
lib.dwt_hip_wp_best2d_batch.argtypes = [_I, _I, _F, _P, _P, _S, _I, _I, _I, _I, _I, _I, _P, _S, _P, _P, _S]
lib.dwt_hip_wp_best2d_batch.restype = _I
lib.dwt_hip_wp_tree2d_batch.argtypes = [_I, _I, _P, _P, _S, _I, _I, _I, _I, _I, _I, _P, _S]
lib.dwt_hip_wp_tree2d_batch.restype = _I


def wp_nodes(size, level):
    """dwt_hip_wp_nodes: ([start], [len]) of the 2^level nodes of `level` of a line of `size` samples, natural order."""
    n = lib.dwt_hip_wp_nodes(size, level, None, None)
    if n < 0:
        raise DwtError("wp_nodes: level %d of a line of %d samples" % (level, size))
    start, length = (_I * n)(), (_I * n)()
    lib.dwt_hip_wp_nodes(size, level, start, length)
    return list(start), list(length)


def wp_freq_order(level):
    """dwt_hip_wp_freq_order: perm[f] = natural index of the node whose band is the f-th lowest (the Gray code)."""
    n = lib.dwt_hip_wp_freq_order(level, None)
    if n < 0:
        raise DwtError("wp_freq_order: level %d" % level)
    perm = (_I * n)()
    lib.dwt_hip_wp_freq_order(level, perm)
    return list(perm)


def wp1d_batch(wavelet, inverse, src, dst, line_stride, elem_stride, n_lines, size, levels):
    """dwt_hip_wp1d_batch: `levels` packet levels of n_lines rows (1 <= levels <= floor(log2 size)); src == dst is in
    place.  Device rows of up to 8192 samples take one launch."""
    _check(lib.dwt_hip_wp1d_batch(wavelet, 1 if inverse else 0, _addr(src), _addr(dst), line_stride, elem_stride, n_lines, size,
                                  levels), "dwt_hip_wp1d_batch")


def wp2d_batch(wavelet, inverse, src, dst, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels):
    """dwt_hip_wp2d_batch: `levels` packet levels of a batch of images (1 <= levels <= min(floor(log2(min size)), 8));
    src == dst is in place.  Dense device images take one launch per level."""
    _check(lib.dwt_hip_wp2d_batch(wavelet, 1 if inverse else 0, _addr(src), _addr(dst), batch_stride, batch, stride_x, stride_y,
                                  size_x, size_y, levels), "dwt_hip_wp2d_batch")


def wp_features1d_batch(features, ptr, line_stride, elem_stride, n_lines, size, level, order, fv, fv_stride, p=2.0):
    """dwt_hip_wp_features1d_batch: the statistics of every node of `level` of transformed packet rows; per row one block
    of 2^level floats per feature of the mask, node order NATURAL or FREQUENCY."""
    _check(lib.dwt_hip_wp_features1d_batch(feature_mask(features), _addr(ptr), line_stride, elem_stride, n_lines, size, level,
                                           order, float(p), _addr(fv), fv_stride), "dwt_hip_wp_features1d_batch")


def wp_features2d_batch(features, ptr, batch_stride, batch, stride_x, size_x, size_y, level, order, fv, fv_stride, p=2.0):
    """dwt_hip_wp_features2d_batch: the same for images; node (ky, kx) at ky * 2^level + kx of a feature's block."""
    _check(lib.dwt_hip_wp_features2d_batch(feature_mask(features), _addr(ptr), batch_stride, batch, stride_x, size_x, size_y,
                                           level, order, float(p), _addr(fv), fv_stride), "dwt_hip_wp_features2d_batch")


def _opt(p):
    return None if p is None else _addr(p)


def wp_best_tree(levels, cost):
    """dwt_hip_wp_best_tree: (tree, total) of a table of 2^(levels+1) node costs in heap order ([0] unused); the tree is a
    list of TREE_WORDS words holding effective bits only.  A tie and a NaN keep the parent.  Host only."""
    cost = [float(c) for c in cost]
    if not 1 <= levels <= TREE_MAX_LEVELS or len(cost) < (2 << levels):
        raise DwtError("wp_best_tree: %d levels, a table of %d costs" % (levels, len(cost)))
    table, tree, total = (C.c_double * len(cost))(*cost), (C.c_uint32 * TREE_WORDS)(), C.c_double()
    if lib.dwt_hip_wp_best_tree(levels, table, tree, C.byref(total)) != 0:
        raise DwtError("wp_best_tree: bad arguments")
    return list(tree), total.value


def wp_tree_leaves(size, levels, tree):
    """dwt_hip_wp_tree_leaves: [(level, index, start, len)] of the leaves of the effective tree, left to right.  Host only."""
    tree = [int(t) for t in tree]
    if len(tree) != TREE_WORDS:
        raise DwtError("wp_tree_leaves: a tree has %d words" % TREE_WORDS)
    words = (C.c_uint32 * TREE_WORDS)(*tree)
    n = lib.dwt_hip_wp_tree_leaves(size, levels, words, None, None, None, None)
    if n < 0:
        raise DwtError("wp_tree_leaves: %d levels over a line of %d samples" % (levels, size))
    out = [(_I * n)() for _ in range(4)]
    lib.dwt_hip_wp_tree_leaves(size, levels, words, *out)
    return list(zip(*(list(o) for o in out)))


def wp_best1d_batch(wavelet, cost, param, src, dst, line_stride, elem_stride, n_lines, size, levels, tree=None,
                    tree_stride=4 * TREE_WORDS, total=None, node_cost=None, cost_stride=None):
    """dwt_hip_wp_best1d_batch: the cost of every node, the best tree of every row and (dst not None) the row in that tree.
    Every output is optional and lies where src lies; strides in bytes (cost_stride None: dense tables).  Device rows of up
    to 8192 samples take one launch; nothing is read back."""
    if cost_stride is None:
        cost_stride = 8 * (2 << levels) if 0 <= levels <= 30 else 0
    _check(lib.dwt_hip_wp_best1d_batch(wavelet, cost, float(param), _addr(src), _opt(dst), line_stride, elem_stride, n_lines, size,
                                       levels, _opt(tree), tree_stride, _opt(total), _opt(node_cost), cost_stride),
           "dwt_hip_wp_best1d_batch")


def wp_tree1d_batch(wavelet, inverse, src, dst, line_stride, elem_stride, n_lines, size, levels, tree, tree_stride=0):
    """dwt_hip_wp_tree1d_batch: the rows in given trees, forward or inverse; tree_stride 0 is one tree for every row.  The
    trees lie where src lies -- except that a list of TREE_WORDS ints (what wp_best_tree returns) is taken for rows in
    either memory space: for device rows it is copied to device memory for the length of the call."""
    tmp = None
    if isinstance(tree, (list, tuple)):
        words = (C.c_uint32 * TREE_WORDS)(*[int(t) for t in tree])
        tree, tree_stride = C.addressof(words), 0
        if lib.dwt_hip_is_device_pointer(_addr(src)):
            tmp = lib.dwt_hip_malloc(4 * TREE_WORDS)
            if not tmp or lib.dwt_hip_memcpy_h2d(tmp, tree, 4 * TREE_WORDS) != 0:
                raise DwtError("wp_tree1d_batch: no device memory for the tree")
            tree = tmp
    try:
        _check(lib.dwt_hip_wp_tree1d_batch(wavelet, 1 if inverse else 0, _addr(src), _addr(dst), line_stride, elem_stride, n_lines,
                                           size, levels, _addr(tree), tree_stride), "dwt_hip_wp_tree1d_batch")
    finally:
        if tmp:
            lib.dwt_hip_sync()
            lib.dwt_hip_free(tmp)


def wp_joint_basis(wavelet, cost, param, src, line_stride, elem_stride, n_lines, size, levels):
    """One tree for all rows: the search for the cost tables alone, the tables summed over the rows on the host in float64
    (row order), wp_best_tree of the sum.  Returns the tree (a list of TREE_WORDS words) for wp_tree1d_batch(...,
    tree_stride=0); src is only read."""
    import numpy as np

    nt = 2 << levels
    table = np.zeros((max(n_lines, 0), nt), np.float64)
    if lib.dwt_hip_is_device_pointer(_addr(src)):
        dev = lib.dwt_hip_malloc(max(table.nbytes, 16))
        if not dev:
            raise DwtError("wp_joint_basis: no device memory for the cost tables")
        try:
            wp_best1d_batch(wavelet, cost, param, src, None, line_stride, elem_stride, n_lines, size, levels, node_cost=dev)
            lib.dwt_hip_sync()
            if table.nbytes and lib.dwt_hip_memcpy_d2h(table.ctypes.data, dev, table.nbytes) != 0:
                raise DwtError("wp_joint_basis: the cost tables could not be read")
        finally:
            lib.dwt_hip_free(dev)
    else:
        wp_best1d_batch(wavelet, cost, param, src, None, line_stride, elem_stride, n_lines, size, levels, node_cost=table)
    joint = np.zeros(nt, np.float64)
    for row in table:
        joint += row
    return wp_best_tree(levels, joint)[0]


# ---- quadtrees of image batches ----------------------------------------------------------------------
def qtree_nodes(levels):
    """the nodes of levels 0 .. `levels` of a quadtree: the length of a cost table"""
    return ((4 << (2 * levels)) - 1) // 3


def wp_best_qtree(levels, cost):
    """dwt_hip_wp_best_qtree: (tree, total) of a table of (4^(levels+1) - 1)/3 node costs in index order (node (ky, kx) of
    level j at (4^j - 1)/3 + ky * 2^j + kx); the tree is a list of QTREE_WORDS words holding effective bits only.  A tie
    and a NaN keep the parent.  Host only."""
    cost = [float(c) for c in cost]
    if not 1 <= levels <= QTREE_MAX_LEVELS or len(cost) < qtree_nodes(levels):
        raise DwtError("wp_best_qtree: %d levels, a table of %d costs" % (levels, len(cost)))
    table, tree, total = (C.c_double * len(cost))(*cost), (C.c_uint32 * QTREE_WORDS)(), C.c_double()
    if lib.dwt_hip_wp_best_qtree(levels, table, tree, C.byref(total)) != 0:
        raise DwtError("wp_best_qtree: bad arguments")
    return list(tree), total.value


def wp_qtree_leaves(size_x, size_y, levels, tree):
    """dwt_hip_wp_qtree_leaves: [(level, ky, kx, x0, y0, w, h)] of the leaves of the effective tree, depth first with the
    children in the order LL, HL, LH, HH.  Host only."""
    tree = [int(t) for t in tree]
    if len(tree) != QTREE_WORDS:
        raise DwtError("wp_qtree_leaves: a quadtree has %d words" % QTREE_WORDS)
    words = (C.c_uint32 * QTREE_WORDS)(*tree)
    n = lib.dwt_hip_wp_qtree_leaves(size_x, size_y, levels, words, *([None] * 7))
    if n < 0:
        raise DwtError("wp_qtree_leaves: %d levels over an image of %d x %d" % (levels, size_x, size_y))
    out = [(_I * n)() for _ in range(7)]
    lib.dwt_hip_wp_qtree_leaves(size_x, size_y, levels, words, *out)
    return list(zip(*(list(o) for o in out)))


def wp_best2d_batch(wavelet, cost, param, src, dst, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, tree=None,
                    tree_stride=4 * QTREE_WORDS, total=None, node_cost=None, cost_stride=None):
    """dwt_hip_wp_best2d_batch: the cost of every node, the best quadtree of every image and (dst not None) the image in
    that tree.  Every output is optional and lies where src lies; strides in bytes (cost_stride None: dense tables).  Dense
    device images take 2 * levels + 2 launches (3 * levels + 2 with dst); nothing is read back."""
    if cost_stride is None:
        cost_stride = 8 * qtree_nodes(levels) if 0 <= levels <= 12 else 0
    _check(lib.dwt_hip_wp_best2d_batch(wavelet, cost, float(param), _addr(src), _opt(dst), batch_stride, batch, stride_x, stride_y,
                                       size_x, size_y, levels, _opt(tree), tree_stride, _opt(total), _opt(node_cost), cost_stride),
           "dwt_hip_wp_best2d_batch")


def wp_tree2d_batch(wavelet, inverse, src, dst, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, tree, tree_stride=0):
    """dwt_hip_wp_tree2d_batch: the images in given quadtrees, forward or inverse; tree_stride 0 is one tree for every
    image.  The trees lie where src lies -- except that a list of QTREE_WORDS ints (what wp_best_qtree returns) is taken
    for images in either memory space: for device images it is copied to device memory for the length of the call."""
    tmp = None
    if isinstance(tree, (list, tuple)):
        words = (C.c_uint32 * QTREE_WORDS)(*[int(t) for t in tree])
        tree, tree_stride = C.addressof(words), 0
        if lib.dwt_hip_is_device_pointer(_addr(src)):
            tmp = lib.dwt_hip_malloc(4 * QTREE_WORDS)
            if not tmp or lib.dwt_hip_memcpy_h2d(tmp, tree, 4 * QTREE_WORDS) != 0:
                raise DwtError("wp_tree2d_batch: no device memory for the tree")
            tree = tmp
    try:
        _check(lib.dwt_hip_wp_tree2d_batch(wavelet, 1 if inverse else 0, _addr(src), _addr(dst), batch_stride, batch, stride_x, stride_y,
                                           size_x, size_y, levels, _addr(tree), tree_stride), "dwt_hip_wp_tree2d_batch")
    finally:
        if tmp:
            lib.dwt_hip_sync()
            lib.dwt_hip_free(tmp)


def wp_joint_qtree(wavelet, cost, param, src, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels):
    """One quadtree for all images, the 2-D twin of wp_joint_basis: the search for the cost tables alone, the tables summed
    over the images on the host in float64 (batch order), wp_best_qtree of the sum.  Returns the tree (a list of
    QTREE_WORDS words) for wp_tree2d_batch(..., tree_stride=0); src is only read."""
    import numpy as np

    nq = qtree_nodes(levels)
    table = np.zeros((max(batch, 0), nq), np.float64)
    args = (wavelet, cost, param, src, None, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels)
    if lib.dwt_hip_is_device_pointer(_addr(src)):
        dev = lib.dwt_hip_malloc(max(table.nbytes, 16))
        if not dev:
            raise DwtError("wp_joint_qtree: no device memory for the cost tables")
        try:
            wp_best2d_batch(*args, node_cost=dev)
            lib.dwt_hip_sync()
            if table.nbytes and lib.dwt_hip_memcpy_d2h(table.ctypes.data, dev, table.nbytes) != 0:
                raise DwtError("wp_joint_qtree: the cost tables could not be read")
        finally:
            lib.dwt_hip_free(dev)
    else:
        wp_best2d_batch(*args, node_cost=table)
    joint = np.zeros(nq, np.float64)
    for row in table:
        joint += row
    return wp_best_qtree(levels, joint)[0]
