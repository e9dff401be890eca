"""``Dataloader`` of the BEV tree: ``Load_Data_new.write_lsq_results`` on the device; the loader classes stay the reference's."""
