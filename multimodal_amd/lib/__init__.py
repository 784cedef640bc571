"""The library's models.  `BetaNMF` (lib/beta_nmf.py) is exported here and loaded on first use: a process that stays with the
default cost never imports the beta path."""


def __getattr__(name):
    if name == 'BetaNMF':
        from .beta_nmf import BetaNMF
        return BetaNMF
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
