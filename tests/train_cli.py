"""The command line of nsd_amd.train as the flag tests read it.  No GPU needed."""


def parse_train_args(argv, monkeypatch):
    """Run nsd_amd.train.main up to the point where it looks for a device; returns the argparse namespace it built there."""
    from nsd_amd import train
    seen = {}

    def stop():
        raise RuntimeError("a device was touched")
    monkeypatch.setattr(train, "init_distributed", stop)
    real = train.argparse.ArgumentParser.parse_args

    def spy(self, *a, **kw):
        seen["args"] = real(self, *a, **kw)
        return seen["args"]
    monkeypatch.setattr(train.argparse.ArgumentParser, "parse_args", spy)
    try:
        train.main(argv)
    except RuntimeError as e:
        assert "device was touched" in str(e)
        seen["reached_device"] = True
    return seen
