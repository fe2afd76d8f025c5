"""ServeConfig.batch_multiclass: off by default, overridable by RDP_SERVE_BATCH_MULTICLASS like every serve field."""


def test_serve_config_batch_multiclass(monkeypatch):
    from robotic_discovery_platform_amd.config import ServeConfig, apply_env
    monkeypatch.delenv("RDP_SERVE_BATCH_MULTICLASS", raising=False)
    assert ServeConfig().batch_multiclass is False
    assert apply_env(ServeConfig(), "serve").batch_multiclass is False
    monkeypatch.setenv("RDP_SERVE_BATCH_MULTICLASS", "1")
    cfg = apply_env(ServeConfig(), "serve")
    assert cfg.batch_multiclass is True
    monkeypatch.setenv("RDP_SERVE_BATCH_MULTICLASS", "0")
    assert apply_env(ServeConfig(), "serve").batch_multiclass is False


def test_pool_policy_reads_the_override(monkeypatch):
    """EnginePool(batch_multiclass=None) follows the environment, an explicit value wins."""
    from robotic_discovery_platform_amd.serve.engine import batch_multiclass_policy
    monkeypatch.delenv("RDP_SERVE_BATCH_MULTICLASS", raising=False)
    assert batch_multiclass_policy(None) is False
    monkeypatch.setenv("RDP_SERVE_BATCH_MULTICLASS", "1")
    assert batch_multiclass_policy(None) is True
    assert batch_multiclass_policy(False) is False
    monkeypatch.setenv("RDP_SERVE_BATCH_MULTICLASS", "0")
    assert batch_multiclass_policy(None) is False
    assert batch_multiclass_policy(True) is True
