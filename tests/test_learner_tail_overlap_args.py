"""hb_noisy_adam_multi checks a gradient-product entry (hb_adam_tensor.gx) before it touches the device: bad calls come back
with a negative code and a message, also on a machine without a GPU (nothing here launches anything)."""


def test_argument_validation_needs_no_gpu():
    import hanabi_hip
    from hanabi_hip import _capi as K

    L = hanabi_hip.lib()
    one = 16      # a non-null, 16-byte aligned fake pointer: validation must reject the call before using it

    def call(n_extra=0, eff_dtype=1, step=one, **kw):
        f = dict(grad=one, grad_dtype=1, grad_ld=512, n=658 * 512, cols=512, gx=one, gdh=one, g_batch=256, g_ldx=704, g_ldh=512)
        f.update(kw)
        tab = (K.HbAdamTensor * (1 + n_extra))()
        for k, v in f.items():
            setattr(tab[n_extra], k, v)
        return L.hb_noisy_adam_multi(tab, 1 + n_extra, step, 0.0, eff_dtype, 1e-3, 0.9, 0.999, 1e-5, None)

    assert call(gdh=None) < 0 and b"null" in L.hb_last_error()
    assert call(grad=None) < 0 and b"null" in L.hb_last_error()
    assert call(step=None) < 0 and b"null" in L.hb_last_error()
    assert call(grad_dtype=0, eff_dtype=0) < 0 and b"grad_dtype" in L.hb_last_error()
    assert call(eff_dtype=2) < 0 and b"eff_dtype" in L.hb_last_error()
    assert call(g_batch=0) < 0 and b"g_batch" in L.hb_last_error()
    assert call(g_batch=257) < 0 and b"g_batch" in L.hb_last_error()
    assert call(cols=508, n=658 * 508) < 0 and b"multiple of 8" in L.hb_last_error()
    assert call(n=0) < 0
    assert call(g_ldx=656) < 0 and b"leading" in L.hb_last_error()      # g_ldx < rows
    assert call(g_ldx=660) < 0 and b"leading" in L.hb_last_error()      # not a multiple of 8
    assert call(g_ldh=504) < 0 and call(grad_ld=510) < 0 and call(grad_ld=514) < 0
    assert call(gx=20) < 0 and b"aligned" in L.hb_last_error()
    assert call(grad=12) < 0 and b"aligned" in L.hb_last_error()
    # the entries stepped beside the product are checked like any hb_noisy_adam_multi table
    assert call(n_extra=1) < 0 and b"tensor 0" in L.hb_last_error()
    # at most one product per launch
    tab = (K.HbAdamTensor * 2)()
    tab[0].gx = tab[1].gx = one
    assert L.hb_noisy_adam_multi(tab, 2, one, 0.0, 1, 1e-3, 0.9, 0.999, 1e-5, None) < 0 and b"at most one" in L.hb_last_error()
