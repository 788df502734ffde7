"""andi_amd — MI355X (gfx950) engine for andi's anchor-distance hot path.

The product is libandihip.so (HIP kernels + C-ABI, include/andi_hip.h); this
package is the thin Python mirror of that interface used by the tests and the
benchmark.
"""
from . import lib, synth  # noqa: F401
from .lib import (AndiHipError, Context, bootstrap, bootstrap_nj, bootstrap_range, bootstrap_tree, Esa, Queries, M_ANI, M_JC, M_KIMURA, M_LOGDET, M_RAW,  # noqa: F401
                  consensus, dist_matrix, dist_rect, distances, estimate, estimate_portable, format_distances, format_distances_rect,
                  match_positions, newick, newick_consensus, newick_transfer, nj, nj_batch, nj_splits, nj_support, nj_transfer,
                  nj_transfer_taxa, tree, tree_batch,
                  LINK, cluster_medoids, cluster_stability, linkage, linkage_batch, linkage_cut, newick_linkage,
                  FILL, complete, complete_batch,
                  DELTA, delta_scores,
                  PLACEMENT, distances_rect, jplace, parse_newick, place,
                  ROOT, newick_rooted, root,
                  FIT, fit, relength,
                  REFINE, REFINE_MOVE, refine, SPR_MOVE, refine_spr,
                  Sketches, screen, screen_select, sketch, sketch_shared,
                  scan_rows, subject_prepare, suffix_array)
