# The reduced stmogen config with the speech-to-gesture control branch, in the scheme of the reference's configs/stmogen/S2G_Beats2_*.py:
# the top-level keys tools/s2g_test.py:592-601 reads to wrap the model; dims match tests/helpers.py CTRL (three layers, two copied).
_base_ = ['stmogen_small.py']

model = dict(model=dict(num_layers=3))
copy_blocks_num, control_cond_feats = 2, 2
condition_encode_cfg = dict(dataset_name='beats2', condition_pre_encode=True, condition_pre_encode_type='wav', control_cond_feats=2,
                            condition_latent_dim=32 * 12, condition_cfg=True)
