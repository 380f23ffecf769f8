"""Host side of the gradient-finish switch (EngineOptions.grad_finish): read from the environment like every other launch-path switch."""


def test_grad_finish_switch_is_read_from_the_environment(monkeypatch):
    from wavenet_autoencoders_amd.options import EngineOptions
    import wavenet_autoencoders_amd.options as opts
    monkeypatch.delenv("WAE_GRAD_FINISH", raising=False)
    assert EngineOptions().grad_finish and EngineOptions.from_env().grad_finish
    monkeypatch.setenv("WAE_GRAD_FINISH", "0")
    assert not EngineOptions.from_env().grad_finish
    monkeypatch.setenv("WAE_GRAD_FINISH", "1")
    assert EngineOptions.from_env().grad_finish
    assert "WAE_GRAD_FINISH" in opts.__doc__
