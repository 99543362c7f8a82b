"""CPU tier of hip.event_voxels, the one route from a caller's configuration (source, flavour, hot-pixel masks, out or scatter only)
to the public binding that serves it.  The twelve bindings are replaced by recorders; the table below is written out by hand from
the ladders the route replaced (MultiStreamSegmenter._ingest, SequenceSegmenter._round, EventBatchBuilder's two scatter sites)."""
import inspect

import pytest

from ess_amd import hip

BINDINGS = ('event_ingest_columns', 'event_ingest_columns_trilinear', 'event_ingest_ring', 'event_ingest_ring_trilinear',
            'event_scatter_ring', 'event_scatter_ring_trilinear', 'event_scatter_ring_rep', 'event_ingest_ring_rep',
            'event_ingest_columns_rep', 'event_ingest_masked', 'event_scatter_store', 'event_ingest_store')

SIGNED, SEPARATE, HISTOGRAM, TRILINEAR = 'signed', 'separate', 'histogram', 'trilinear'

# (source, flavour, masks given, out given) -> the binding.  Not reached by any ladder, and absent: the column source scatter-only
# without masks.  (Trilinear with a non-signed representation is no flavour of this list.)
EXPECTED = {
    ('ring', SIGNED, False, True): 'event_ingest_ring',
    ('ring', SEPARATE, False, True): 'event_ingest_ring_rep',
    ('ring', HISTOGRAM, False, True): 'event_ingest_ring_rep',
    ('ring', TRILINEAR, False, True): 'event_ingest_ring_trilinear',
    ('ring', SIGNED, False, False): 'event_scatter_ring',
    ('ring', SEPARATE, False, False): 'event_scatter_ring_rep',
    ('ring', HISTOGRAM, False, False): 'event_scatter_ring_rep',
    ('ring', TRILINEAR, False, False): 'event_scatter_ring_trilinear',
    ('ring', SIGNED, True, True): 'event_ingest_masked',
    ('ring', SEPARATE, True, True): 'event_ingest_masked',
    ('ring', HISTOGRAM, True, True): 'event_ingest_masked',
    ('ring', TRILINEAR, True, True): 'event_ingest_masked',
    ('ring', SIGNED, True, False): 'event_ingest_masked',
    ('ring', SEPARATE, True, False): 'event_ingest_masked',
    ('ring', HISTOGRAM, True, False): 'event_ingest_masked',
    ('ring', TRILINEAR, True, False): 'event_ingest_masked',
    ('columns', SIGNED, False, True): 'event_ingest_columns',
    ('columns', SEPARATE, False, True): 'event_ingest_columns_rep',
    ('columns', HISTOGRAM, False, True): 'event_ingest_columns_rep',
    ('columns', TRILINEAR, False, True): 'event_ingest_columns_trilinear',
    ('columns', SIGNED, True, True): 'event_ingest_masked',
    ('columns', SEPARATE, True, True): 'event_ingest_masked',
    ('columns', HISTOGRAM, True, True): 'event_ingest_masked',
    ('columns', TRILINEAR, True, True): 'event_ingest_masked',
    ('columns', SIGNED, True, False): 'event_ingest_masked',
    ('columns', SEPARATE, True, False): 'event_ingest_masked',
    ('columns', HISTOGRAM, True, False): 'event_ingest_masked',
    ('columns', TRILINEAR, True, False): 'event_ingest_masked',
    ('store', SIGNED, False, False): 'event_scatter_store',
    ('store', SEPARATE, False, False): 'event_scatter_store',
    ('store', HISTOGRAM, False, False): 'event_scatter_store',
    ('store', TRILINEAR, False, False): 'event_scatter_store',
    ('store', SIGNED, False, True): 'event_ingest_store',
    ('store', SEPARATE, False, True): 'event_ingest_store',
    ('store', HISTOGRAM, False, True): 'event_ingest_store',
    ('store', TRILINEAR, False, True): 'event_ingest_store',
    ('store', SIGNED, True, True): 'event_ingest_store',
    ('store', SEPARATE, True, True): 'event_ingest_store',
    ('store', HISTOGRAM, True, True): 'event_ingest_store',
    ('store', TRILINEAR, True, True): 'event_ingest_store',
    ('store', SIGNED, True, False): 'event_ingest_store',
    ('store', SEPARATE, True, False): 'event_ingest_store',
    ('store', HISTOGRAM, True, False): 'event_ingest_store',
    ('store', TRILINEAR, True, False): 'event_ingest_store',
}

# the word each binding is handed for a flavour: the representation (masked: beside trilinear), the store's flavour word
REP = {SIGNED: 0, SEPARATE: 1, HISTOGRAM: 2, TRILINEAR: 0}
STORE_FLAVOUR = {SIGNED: 0, SEPARATE: 1, HISTOGRAM: 2, TRILINEAR: 3}
WORDS = {'ring': ('rows', 'starts', 'counts', 'formats'), 'columns': ('counts', 'formats'), 'store': ('starts', 'counts', 'formats')}


@pytest.fixture
def calls(monkeypatch):
    """every binding a recorder: (name, its arguments by parameter name, defaults filled in)"""
    seen = []
    for name in BINDINGS:
        signature = inspect.signature(getattr(hip, name))

        def recorder(*args, _name=name, _signature=signature, **kwargs):
            bound = _signature.bind(*args, **kwargs)
            bound.apply_defaults()
            seen.append((_name, dict(bound.arguments)))
            return _name
        monkeypatch.setattr(hip, name, recorder)
    return seen


def test_the_constants_the_table_is_written_in():
    assert (hip.EVENT_REP_SIGNED, hip.EVENT_REP_SEPARATE, hip.EVENT_REP_HISTOGRAM) == (0, 1, 2)
    assert (hip.EVENT_STORE_SIGNED, hip.EVENT_STORE_SEPARATE, hip.EVENT_STORE_HISTOGRAM, hip.EVENT_STORE_TRILINEAR) == (0, 1, 2, 3)
    assert len(EXPECTED) == 3 * 4 * 2 * 2 - 4


@pytest.mark.parametrize('case', sorted(EXPECTED), ids=lambda c: '-'.join(str(v) for v in c))
def test_the_route_calls_the_binding_the_ladders_called_and_hands_everything_on(calls, case):
    kind, flavour, masked, with_out = case
    tri = flavour == TRILINEAR
    out = 'OUT' if with_out else None
    masks = ('MASKS', 'MASK_OF', (3, 5)) if masked else None
    store = dict(total=4096, window_capacity=512) if kind == 'store' else {}
    got = hip.event_voxels(kind, ('T', 'X', 'Y', 'P'), WORDS[kind], out, 'ACC', representation=REP[flavour], trilinear=tri, maps='MAPS',
                           map_of='MAP_OF', masks=masks, **store)
    assert len(calls) == 1
    name, args = calls[0]
    assert name == EXPECTED[case] and got == name
    # the source, the grids and the sums arrive under their own names
    assert (args['t'], args['x'], args['y'], args['p']) == ('T', 'X', 'Y', 'P')
    for word in WORDS[kind]:
        assert args[word] == word
    if name == 'event_ingest_masked' and kind == 'columns':
        assert args['rows'] is None and args['starts'] is None
    assert args['acc'] == 'ACC'
    assert args.get('out') == out  # (the scatter-only bindings have no out)
    # the flavour: maps and map_of reach a trilinear call alone
    if 'maps' in args:
        assert (args['maps'], args['map_of']) == (('MAPS', 'MAP_OF') if tri else (None, None))
    else:
        assert not tri
    if 'flavour' in args:
        assert args['flavour'] == STORE_FLAVOUR[flavour]
        assert (args['total'], args['window_capacity']) == (4096, 512)
    elif name == 'event_ingest_masked':
        assert (args['representation'], bool(args['trilinear'])) == (REP[flavour], tri)
    elif 'representation' in args:
        assert args['representation'] == REP[flavour] != 0
    else:
        assert flavour in (SIGNED, TRILINEAR)
    # the masks: the triple a configured caller holds, or none at all
    if 'masks' in args:
        assert (args['masks'], args['mask_of'], args['mask_size']) == (('MASKS', 'MASK_OF', (3, 5)) if masked else (None, None, None))
    else:
        assert not masked


def test_the_one_combination_no_ladder_reached_is_refused_not_invented(calls):
    with pytest.raises(hip.EssHipError, match='scatter only'):
        hip.event_voxels('columns', ('T', 'X', 'Y', 'P'), WORDS['columns'], None, 'ACC')
    assert calls == []
