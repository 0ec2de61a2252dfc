"""A module that only re-exports, and still takes an assignment the way the module that defined everything did."""
import sys
import types


class ReExporting(types.ModuleType):
    """Assigning a re-exported name on the facade (`monkeypatch.setattr(hip, 'recommended_dims', ...)`, what the tests do to
    force a padded box) assigns it in the module it came from as well: that is where the code that calls it looks it up.  The
    home of a name is found at its first assignment, while the facade still holds the home module's own object, and kept: the
    assignment that undoes the first one is passed on too."""

    def __setattr__(self, name, value):
        homes = self.__dict__.setdefault('_homes', {})
        if name not in homes:
            old = self.__dict__.get(name)
            home = sys.modules.get(getattr(old, '__module__', None) or '')
            homes[name] = home if home is not None and home is not self and home.__dict__.get(name) is old else None
        if homes[name] is not None:
            setattr(homes[name], name, value)
        super().__setattr__(name, value)
