"""What the slide-dataset tests share: the fixture slide and its two position trees under tests/golden/files/, and Loupe
annotation CSVs written from the trees' own barcodes (every third in-tissue spot is left without an annotation, one
out-of-tissue barcode gets one, so that 'annotated' and 'in tissue' differ in both directions)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FILES = os.path.join(HERE, 'golden', 'files')
SLIDE = os.path.join(FILES, 'wsi_slide.png')
SR1 = os.path.join(FILES, 'wsi_sr1')
SR2 = os.path.join(FILES, 'wsi_sr2')
CLASS_NAMES = ('cortex', 'medulla', 'stroma')


def write_annots(tmp_path):
    """[annotation CSV of SR1, of SR2] under tmp_path.  SR1's names two of the classes, SR2's all three: `classes` is the union."""
    from gridnext_amd import imgprocess as IP
    files = []
    for k, srd in enumerate((SR1, SR2)):
        df = IP.visium_get_positions(srd)
        lines = ['Barcode,region']
        n = 0
        for barcode, row in df.iterrows():
            if int(row['in_tissue']) == 1:
                n += 1
                if n % 3 == 0:
                    continue                                   # an in-tissue spot without an annotation
                lines.append('%s,%s' % (barcode, CLASS_NAMES[(n + k) % (2 + k)]))
            else:
                lines.append('%s,%s' % (barcode, CLASS_NAMES[0]))   # annotated, but not in tissue: never an item
        path = os.path.join(str(tmp_path), 'annot_%d.csv' % k)
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
        files.append(path)
    return files


def decoded():
    from PIL import Image
    return np.array(Image.open(SLIDE))
