"""The workspaces of the pair-list satellites (csrc/segsort.h: boot, shift, stack, conformal, prop) as the libraries answer
them on the host -- no GPU needed.  Every literal was recorded from the build of the commit BEFORE the six private copies of
the sort-workspace carve moved onto segsort_carve, so a change of the carve, of a file's own buffers behind it or of a
limit cannot pass quietly.  n: none, one, around the second radix tile (1,024 / 1,025), around every file's own chunk (256
prop, 2,048 shift, 4,096 boot and stack), the x100 graph's 183,400 patients x 50 labs, and the largest n taken (2^31 - 1;
prop takes one fewer).  The other arguments: the smallest shape, a usual one, and the limits."""
import pytest

BIG = 2 ** 31 - 1
NS = (0, 1, 256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 183400 * 50, BIG)

BOOT = {
    (1, 1, 0): [3072, 3072, 6912, 8192, 22272, 24576, 43776, 46080, 86784, 89344, 193078528, 45215646720],
    (50, 1000, 1): [163072, 163072, 166912, 168192, 182272, 184576, 203776, 206080, 246784, 409344, 551175168,
                    129068172288],
    (2048, 4096, 1): [658432, 658432, 662272, 663552, 677632, 679936, 699136, 701440, 742144, 1400064, 1660286208,
                      388779475968],
}
SHIFT = {
    (1, 0): [4096, 4096, 9984, 11264, 31488, 33792, 61184, 63488, 120576, 123136, 266492672, 62408099328],
    (50, 1000): [327936, 327936, 333824, 335104, 355328, 357632, 385024, 511488, 568576, 694784, 821965056, 192431723520],
    (2048, 4096): [34082560, 34082560, 34088448, 34089728, 34109952, 34112256, 34139648, 34649856, 34706944, 35217408,
                   2574457344, 595017614592],
}
STACK_SUMS = {
    (1, 1, 1, 1): [3072, 3072, 6144, 7168, 18432, 20480, 35840, 37888, 70656, 72704, 156004352, 36533437952],
    (50, 4, 2, 5): [90880, 90880, 93952, 94976, 106240, 108288, 123648, 125696, 158720, 160768, 156164096, 36550302976],
    (2048, 16, 4, 8): [46140416, 46140416, 46143488, 46144512, 46155776, 46157824, 46173184, 46175232, 46208256, 46210304,
                       202410496, 36642489600],
}
STACK_SCORES = {
    (1, 1): [3072, 3072, 6144, 7168, 18432, 20480, 35840, 37888, 70656, 72704, 155986432, 36529243648],
    (50, 4): [12544, 12544, 15616, 16640, 27904, 29952, 45312, 47360, 80128, 82176, 155996160, 36529253120],
    (512, 64): [1575936, 1575936, 1579008, 1580032, 1591296, 1593344, 1608704, 1610752, 1643520, 1645568, 157559296,
                36530816256],
}
SOS_BY_N = [2560, 2560, 7680, 8704, 26112, 28160, 51712, 53760, 102912, 104960, 229256448, 53688140800]
SOS = {(1,): SOS_BY_N, (200,): SOS_BY_N, (32768,): SOS_BY_N}          # the segment count sizes nothing
CF_FIT = {
    (1, 1): [6912, 6912, 13568, 15104, 38144, 40704, 71936, 74496, 139520, 142080, 302620672, 70868013824],
    (50, 4): [10752, 10752, 17408, 18944, 41984, 44544, 75776, 78336, 143360, 145920, 302624512, 70868017664],
    (2048, 16): [700672, 700672, 707328, 708864, 731904, 734464, 765696, 768256, 833280, 835840, 303314432, 70868707584],
}
COV_BY_N = [2560, 2560, 5632, 6656, 17920, 19968, 35328, 37376, 70144, 72192, 155896576, 36508271616]
CF_COV = {(1, 1): COV_BY_N, (50, 4): COV_BY_N, (512, 64): COV_BY_N}   # the cells size nothing
# prop refuses n = 2^31 - 1 (the last entry of NS: 0 bytes); the entry after it is n = 2^31 - 2
PROP = {
    (1,): [3328, 3328, 6400, 7424, 18944, 20992, 36352, 38400, 71680, 73728, 157616640, 0, 36910925568],
    (50,): [5632, 5632, 8704, 9728, 21248, 23296, 38912, 40960, 73984, 76032, 157618944, 0, 36910927872],
    (512,): [32000, 32000, 35072, 36096, 47360, 49408, 65024, 67072, 100352, 102400, 157645312, 0, 36910953984],
}

# (module, symbol, {other arguments: bytes by n in NS}, refused (n, other arguments))
CASES = {
    "boot_sums": ("boot_ops", "mmg_boot_sums_ws_bytes", BOOT,
                  [(-1, 50, 1000, 1), (BIG + 1, 50, 1000, 1), (100, 0, 1000, 1), (100, 2049, 1000, 1), (100, 50, 0, 1),
                   (100, 50, 4097, 1)]),
    "shift_stats": ("shift_ops", "mmg_shift_stats_ws_bytes", SHIFT,
                    [(-1, 50, 1000), (BIG + 1, 50, 1000), (100, 0, 1000), (100, 2049, 1000), (100, 50, -1),
                     (100, 50, 4097)]),
    "stack_sums": ("stack_ops", "mmg_stack_sums_ws_bytes", STACK_SUMS,
                   [(-1, 50, 4, 2, 5), (BIG + 1, 50, 4, 2, 5), (100, 0, 4, 2, 5), (100, 2049, 1, 2, 5), (100, 50, 0, 2, 5),
                    (100, 50, 65, 2, 5), (100, 2048, 17, 2, 5), (100, 50, 4, 0, 5), (100, 50, 4, 5, 5), (100, 50, 4, 2, 0),
                    (100, 50, 4, 2, 9)]),
    "stack_scores": ("stack_ops", "mmg_stack_scores_ws_bytes", STACK_SCORES,
                     [(-1, 50, 4), (BIG + 1, 50, 4), (100, 0, 4), (100, 2049, 1), (100, 50, 0), (100, 50, 65),
                      (100, 2048, 17)]),
    "seg_order_stats": ("conformal_ops", "mmg_seg_order_stats_ws_bytes", SOS,
                        [(-1, 200), (BIG + 1, 200), (100, 0), (100, 32769)]),
    "cf_fit": ("conformal_ops", "mmg_cf_fit_ws_bytes", CF_FIT,
               [(-1, 50, 4), (BIG + 1, 50, 4), (100, 0, 4), (100, 2049, 1), (100, 50, 0), (100, 50, 65), (100, 2048, 17)]),
    "cf_coverage": ("conformal_ops", "mmg_cf_coverage_ws_bytes", CF_COV,
                    [(-1, 50, 4), (BIG + 1, 50, 4), (100, 0, 4), (100, 2049, 1), (100, 50, 0), (100, 50, 65),
                     (100, 2048, 17)]),
    "prop_pair_sums": ("prop_ops", "mmg_prop_pair_sums_ws_bytes", PROP,
                       [(-1, 50), (BIG, 50), (BIG + 1, 50), (100, 0), (100, 513)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_workspace_bytes_are_the_recorded_ones(name):
    import importlib
    import mmgnn  # noqa: F401
    module, symbol, table, refused = CASES[name]
    ws = getattr(importlib.import_module(f"mmgnn.{module}").load(), symbol)
    ns = NS + (BIG - 1,) if name == "prop_pair_sums" else NS
    for other, want in table.items():
        assert len(want) == len(ns)
        for n, bytes_ in zip(ns, want):
            assert ws(n, *other) == bytes_, (n, other)
    for args in refused:
        assert ws(*args) == 0, args
