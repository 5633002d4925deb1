"""Image databases by name: the reference's twenty 'bus_<split>' sets, each read from cfg.DATA_DIR when asked for."""
from .bus import bus

SPLITS = tuple(['%s_train%s' % (kind, size) for kind in ('s', 'ws') for size in ('', '_10', '_50', '_100', '_200', '_400', '_600')]
               + ['train', 'reduced_ws_train', 'test', 'test_normal', 's_train_datasetB', 'test_datasetB'])


def list_imdbs():
    return ['bus_' + split for split in SPLITS]


def get_imdb(name):
    """The image database called `name` ('bus_<split>'); KeyError for any other name."""
    if not name.startswith('bus_') or name[4:] not in SPLITS:
        raise KeyError("no image database is called %r (see list_imdbs())" % (name,))
    return bus(name[4:])
