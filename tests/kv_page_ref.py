"""What the operator references share about page offsets that need more than 32 bits (qkv_post_ref, prefill_attn_ref, decode_proj_ref: their relocated cases) -- plain
Python, no GPU needed.  A KV pool is [page][KV][64][D] bf16; page p starts p * KV * 64 * D elements into it.  The relocated cases lay their pages out from the first page
at or above 2^31 (one case per family: 2^30) elements of pools of POOL_ELEMS elements; the PAGE_MUTATIONS are wrong kernels that form that offset in 32 bits."""

POOL_ELEMS = (1 << 31) + (1 << 24)  # elements of each pool of the relocated cases: just over 2^31, room for every case's pages behind it
# the identity on the small pools of the references' lists, wrong on the relocated cases
PAGE_MUTATIONS = ("page_elem_mod_2_31", "page_byte_mod_2_32", "page_byte_int32")


def first_page_above(elems, page_elems):
    """the first page whose element offset is >= elems"""
    return -(-elems // page_elems)


def wrap_page_offset(off, mut):
    """the element offset `off` of a page inside its pool as a kernel that forms it in 32 bits would see it.  page_elem_mod_2_31: the element offset mod 2^31;
    page_byte_mod_2_32: the byte offset (2 bytes per element) in an unsigned 32-bit register; page_byte_int32: the byte offset in a SIGNED one -- negative, i.e. in
    front of the pool, from 2^31 bytes on.  The first two are the identity below 2^31 elements (arithmetic, not a gap: no 32-bit unsigned form is wrong there), the third
    is wrong from 2^30 elements on."""
    if mut == "page_elem_mod_2_31":
        return off % (1 << 31)
    if mut == "page_byte_mod_2_32":
        return (2 * off) % (1 << 32) // 2
    if mut == "page_byte_int32":
        return ((2 * off + (1 << 31)) % (1 << 32) - (1 << 31)) // 2
    return off
