"""The overlap queries' row for the frame of the list-driven tests (pair_list_harness.Query), as the four rows of
pair_list_harness.QUERIES state the older queries: a plain module that the overlap tests, tests/overlap_graph_check.py and
tests/tools/overlap_fuzz.py import.  It loads numpy references only, never the library."""
import pair_list_harness
from overlap_ref import BAD_PAIR, OVERLAP_DT, poly_overlaps, rect_overlaps, same

OVERLAPS = pair_list_harness.Query("overlaps", (OVERLAP_DT,), (same,), ("records",), BAD_PAIR, "poly_pair_overlaps", poly_overlaps, "rect_pair_overlaps",
                                   rect_overlaps)
