"""Data layers (reference code/lib/roi_data_layer): roidb mini-batches as device blobs, the image blob of a whole
batch built by one device op (utils.blob.image_batch_blob)."""
