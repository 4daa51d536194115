"""Hand-worked cases of tests/edges_from_lists_model.py (no GPU): the order rule of
rrtx_graph_edges_append_lists, written out edge by edge."""
import numpy as np

from edges_from_lists_model import edges_from_lists


def _u8(*v):
    return np.asarray(v, dtype=np.uint8)


def test_blocked_out_edge_with_a_free_in_edge():
    # one sample (node 7), one neighbour (node 2): out blocked, in free -> both edges, the out-edge blocked
    m = edges_from_lists([0, 1], [2], [1.5], [2.5], _u8(1), _u8(0), [7])
    assert m["start"].tolist() == [7, 2] and m["end"].tolist() == [2, 7]
    assert m["cost"].tolist() == [1.5, 2.5]
    assert m["blocked"].tolist() == [True, False]
    assert m["row_first"].tolist() == [0, 2]


def test_both_blocked_keeps_only_the_out_edge():
    m = edges_from_lists([0, 2], [2, 3], [1.0, 4.0], [1.0, 4.0], _u8(2, 0), _u8(1, 0), [9])
    # entry 0: both blocked (a flag byte of 2 counts) -> out-edge only, blocked; entry 1: both free -> out, in
    assert m["start"].tolist() == [9, 9, 3] and m["end"].tolist() == [2, 3, 9]
    assert m["cost"].tolist() == [1.0, 4.0, 4.0]
    assert m["blocked"].tolist() == [True, False, False]
    assert m["row_first"].tolist() == [0, 3]


def test_a_sample_that_was_not_inserted_and_an_empty_row():
    # three samples: 0 inserted as node 5 with one entry, 1 not inserted (its entry yields nothing), 2 inserted, empty row
    m = edges_from_lists([0, 1, 2, 2], [0, 1], [1.0, 2.0], [1.0, 2.0], _u8(0, 0), _u8(0, 0), [5, -1, 6])
    assert m["start"].tolist() == [5, 0] and m["end"].tolist() == [0, 5]
    assert m["row_first"].tolist() == [0, 2, 2, 2]
    assert m["dropped"] == 0


def test_a_dropped_self_list_entry():
    # lists among the batch: sample 2 lists samples 0 and 1; sample 1 was not inserted, so that entry is dropped
    m = edges_from_lists([0, 0, 1, 3], [0, 0, 1], [3.0, 1.0, 2.0], [3.5, 1.5, 2.5], _u8(0, 0, 0), _u8(0, 1, 0),
                         [10, -1, 12], idx_is_batch=True)
    # row 1 is not inserted (its entry is not even looked at); row 2: entry (0 -> node 10) out only (in blocked), entry
    # (1 -> not inserted) dropped
    assert m["start"].tolist() == [12] and m["end"].tolist() == [10]
    assert m["cost"].tolist() == [1.0]
    assert m["blocked"].tolist() == [False]
    assert m["row_first"].tolist() == [0, 0, 0, 1]
    assert m["dropped"] == 1


def test_nothing_inserted_and_no_samples():
    m = edges_from_lists([0, 1], [3], [1.0], [1.0], _u8(0), _u8(0), [-1])
    assert m["start"].shape == (0,) and m["row_first"].tolist() == [0, 0]
    m = edges_from_lists([0], np.zeros(0, np.int32), np.zeros(0), np.zeros(0), _u8(), _u8(), np.zeros(0, np.int32))
    assert m["start"].shape == (0,) and m["row_first"].tolist() == [0]


def test_distinct_costs_and_order_within_a_row():
    m = edges_from_lists([0, 2], [4, 1], [1.0, 2.0], [10.0, 20.0], _u8(0, 0), _u8(0, 0), [8])
    assert m["start"].tolist() == [8, 4, 8, 1] and m["end"].tolist() == [4, 8, 1, 8]
    assert m["cost"].tolist() == [1.0, 10.0, 2.0, 20.0]
